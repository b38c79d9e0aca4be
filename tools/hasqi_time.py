#!/usr/bin/env python
"""Device time of HASQI v2 as a training target (nele_metric_hasqi_var) and what it costs inside run_epoch.

    python tools/hasqi_time.py [--out profiles/hasqi/time.json] [--skip-epoch]

(a) phase 0 beside nele_metric_haspi_quality of the same build (the one-shot HASPI v1 + HASQI chain, unchanged), (b) phase 4 alone -
what a cached epoch pays per example - at B = 256 x 4 s and B = 32 x 4 s: HIP events around each call, median of ``--calls`` calls, the
three candidates measured in turn, three such rounds (``rounds``: the median of each round; ``median_ms`` their median, ``spread_ms``
their range).  (c) run_epoch (2 batches of 32 x 4 s with pre-enhanced examples, 'siib&haspi&estoi'): wall time between device
synchronisations of epochs 2-4 after a warm-up epoch, without D_Qua, with D_Qua on targets that come with the batches, and with
D_Qua on HASQI targets enqueued on the features / ESTOI stream or behind HASPI's degraded half, each with the clean-signal cache off and
on; three rounds over all configurations in turn."""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn, calls):
    import torch
    t = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1))
    return statistics.median(t)


def _summary(rounds):
    return {'rounds': rounds, 'median_ms': statistics.median(rounds), 'spread_ms': max(rounds) - min(rounds)}


def calls_part(B, L, calls):
    import numpy as np
    import torch
    from nele_gan_amd import metrics as mt
    from nele_gan_amd import synth
    c, v = synth.batch(8, L, start=6000)
    idx = np.arange(B) % 8
    x = torch.from_numpy(np.ascontiguousarray(c[idx])).cuda()
    y = torch.from_numpy(np.ascontiguousarray((c + 0.5 * v)[idx].astype(np.float32))).cuda()
    ids = torch.arange(B, device='cuda')
    sp = mt.HasqiSplit(x, noise='utterance', seed=0, utt_ids=ids)
    sp.clean_part()
    cand = {'haspi_quality_one_shot': lambda: mt.batch_haspi_quality(x, y, 16000, noise=True, seed=0),
            'hasqi_phase0': lambda: mt.batch_hasqi(x, y, 16000, noise='utterance', seed=0, utt_ids=ids),
            'hasqi_phase0_noise_off': lambda: mt.batch_hasqi(x, y, 16000, noise=False),
            'hasqi_phase4': lambda: sp.degraded_part(y)}
    for fn in cand.values():
        fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in cand}
    for _ in range(3):
        for k, fn in cand.items():
            rounds[k].append(_timed(fn, calls))
    return {k: _summary(r) for k, r in rounds.items()}


def epoch_part(B, L, nb):
    import numpy as np
    import torch
    from nele_gan_amd import quality, synth
    from nele_gan_amd.train_nele import GanTrainer
    c, v = synth.batch(B * nb, L, start=7000)
    drc = np.stack([np.convolve(r, [1.0, -0.6], mode='same') for r in c]).astype(np.float32)
    qua = torch.full((B, 2), 0.5, device='cuda')

    def batches(given):
        out = []
        for k in range(nb):
            s = slice(k * B, (k + 1) * B)
            b = {'clean': torch.from_numpy(c[s]).cuda(), 'noise': torch.from_numpy(v[s]).cuda(), 'drc': torch.from_numpy(drc[s]).cuda(),
                 'names': ['u%d.wav' % i for i in range(k * B, (k + 1) * B)], 'ids': torch.arange(k * B, (k + 1) * B, device='cuda')}
            if given:
                b['qua'], b['drc_qua'] = qua, qua
            out.append(b)
        return out
    kinds = {'no_dqua': (False, None, False), 'dqua_given_targets': (True, None, True),
             'dqua_hasqi_on_features_stream': (True, 'estoi', False), 'dqua_hasqi_behind_haspi': (True, 'haspi', False)}
    rounds = {}
    for rnd in range(3):
        for name, (use_q, stream, given) in kinds.items():
            for cache in (False, True):
                tr = GanTrainer('siib&haspi&estoi', use_quality=use_q, quality_scorer=quality.HasqiScorer() if stream else None)
                if stream:
                    tr.quality_stream = stream
                if cache:
                    tr.enable_clean_cache()
                train = batches(given)
                t = []
                for ep in (1, 2, 3, 4):
                    random.seed(ep)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    tr.run_epoch(ep, train, (), d_batch=B)
                    torch.cuda.synchronize()
                    t.append(1e3 * (time.perf_counter() - t0))
                rounds.setdefault('%s/cache_%s' % (name, 'on' if cache else 'off'), []).append(statistics.median(t[1:]))
                del tr
                torch.cuda.empty_cache()
    return {k: _summary(r) for k, r in rounds.items()}


def main():
    from nele_gan_amd import _lib
    from nele_gan_amd import metrics as mt
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hasqi', 'time.json'))
    ap.add_argument('--calls', type=int, default=7)
    ap.add_argument('--skip-epoch', action='store_true')
    a = ap.parse_args()
    res = {'device': _lib.device_info(), 'calls_per_round': a.calls, 'call_ms': {}}
    for B in (256, 32):
        res['call_ms']['%d x 64000' % B] = r = calls_part(B, 64000, a.calls)
        r['clean_state_bytes_per_utterance'] = sum(nb for (_o, st, nb) in mt.CleanStateCache._sections('hasqi', 1, 64000, 16000) if st > 0)
        print(B, json.dumps(r), flush=True)
    if not a.skip_epoch:
        res['run_epoch_ms'] = {'shape': '2 batches of 32 x 64000, siib&haspi&estoi, pre-enhanced examples', 'configs': epoch_part(32, 64000, 2)}
        print(json.dumps(res['run_epoch_ms']), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
