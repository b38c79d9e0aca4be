#!/usr/bin/env python
"""Does it matter which energy normalisation the generator is trained for?  And what do the prefix kernels cost?

study   One generator per mode ('utterance': the reference's sums over the whole utterance; 'prefix': the causal form the real-time path
        emits) trained with ``GanTrainer(norm=...).run_epoch`` for --epochs epochs on the low-pass-noise corpus of tools/learn_curve.py
        (same seed, bf16 operands), then BOTH generators' validation output scored under BOTH normalisations with the true raw
        SIIB / HASPI / ESTOI: the four cells trained x evaluated, plus the objective of tools/learn_curve.py (mean over metrics of
        (1 - mapped mean)^2) per cell.  No threshold: two float32 seeds of this loop end 0.013 apart in that objective (README), one
        pair of runs records numbers, it does not rank the modes.
timing  nele_energy_norm_prefix_fwd / _bwd against nele_energy_norm_fwd / _bwd on the same tensors at (B, T) = (256, 251), (32, 251),
        (128, 501): medians over --reps repetitions of --inner back-to-back launches between two HIP events, the two kernels
        alternating in one process, after warm-up; and GanTrainer.canonical_step in both modes at B = 256, L = 64 000.

usage: python tools/prefix_norm_study.py [--epochs 30] [--only study,timing] [--out profiles/prefix_norm/study.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from learn_curve import MAPS, batches_of, objective             # noqa: E402
from nele_gan_amd import ops, synth                             # noqa: E402
from nele_gan_amd.train_nele import GanTrainer                  # noqa: E402

MODES = ('utterance', 'prefix')


def score(tr, valid, norm):
    """mean raw metrics (and their mapped means) of the validation set enhanced by tr.G under ``norm``"""
    keep, tr.norm = tr.norm, norm
    try:
        rows = []
        for b in valid:
            f = tr.features(b['clean'], b['noise'])
            enh = tr.generate(f['clean_band'], f['noise_band'], f['clean_spec'])
            rows.append(tr.true_metrics(b['clean'], enh, b['noise'], norm=False, utt_ids=b['ids']))
        raw = torch.cat(rows).double()
    finally:
        tr.norm = keep
    mapped = {m: float((1.0 / (1.0 + torch.exp(-MAPS[m][0] * (raw[:, i] - MAPS[m][1])))).mean()) for i, m in enumerate(tr.metrics)}
    return {'raw': dict(zip(tr.metrics, raw.mean(dim=0).tolist())), 'mapped': mapped, 'objective': objective(mapped)}


def study(a):
    c, v = synth.batch(a.utts, a.length, start=0, noise_tilt=a.noise_tilt)
    cv, vv = synth.batch(a.valid, a.length, start=100000, noise_tilt=a.noise_tilt)
    train = batches_of(torch.from_numpy(c).cuda(), torch.from_numpy(v).cuda(), a.batch, 0)
    valid = batches_of(torch.from_numpy(cv).cuda(), torch.from_numpy(vv).cuda(), max(a.batch, 64), 100000)
    out = {'epochs': a.epochs, 'seed': a.seed, 'precision': a.precision, 'cells': {}, 'curves': {}, 'seconds': {}}
    for mode in MODES:
        tr = GanTrainer(a.metrics, seed=a.seed, norm=mode)
        tr.G.precision = tr.D.precision = a.precision
        t0 = time.perf_counter()
        curve = []
        for ep in range(1, a.epochs + 1):
            res = tr.run_epoch(ep, train, valid, d_batch=a.batch)
            curve.append({'epoch': ep, 'valid': res['valid'], 'objective': objective(res['valid_mapped']),
                          'g_loss': None if res['g_loss'] is None else float(res['g_loss'])})
        torch.cuda.synchronize()
        out['seconds'][mode] = time.perf_counter() - t0
        out['curves'][mode] = curve                             # (validated under the trainer's own mode)
        for ev in MODES:
            out['cells']['trained_%s/evaluated_%s' % (mode, ev)] = score(tr, valid, ev)
            print('trained %-9s evaluated %-9s %s' % (mode, ev, json.dumps(out['cells']['trained_%s/evaluated_%s' % (mode, ev)])), flush=True)
        tr.check_status()
        del tr
    return out


def _events(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner                    # us per launch


def timing(a):
    g = torch.Generator(device='cuda').manual_seed(1)
    P, IP = 1.0 / 6, 6.0
    res = {'unit': 'us per launch (median of %d x %d back-to-back launches between HIP events)' % (a.reps, a.inner), 'kernels': {}}
    for B, T in ((256, 251), (32, 251), (128, 501)):
        clean = torch.rand((B, T, 64), device='cuda', generator=g) * 0.4 + 0.1
        noise = torch.rand((B, T, 64), device='cuda', generator=g) * 0.4 + 0.1
        mask = torch.exp(3.2 * torch.tanh(torch.randn((B, T, 64), device='cuda', generator=g)))
        ddin = torch.randn((B, 64, T, 4), device='cuda', generator=g)
        beta2, s2u, din_u, _ = ops.energy_norm_fwd(clean, mask, noise, P, IP)
        ratio, s2p, din_p, _ = ops.energy_norm_prefix_fwd(clean, mask, noise, P, IP)
        fns = {'utterance_fwd': lambda: ops.energy_norm_fwd(clean, mask, noise, P, IP),
               'prefix_fwd': lambda: ops.energy_norm_prefix_fwd(clean, mask, noise, P, IP),
               'utterance_alpha2': lambda: ops.energy_norm_fwd(clean, mask, None, P, IP, want_din=False, want_alpha2=True),
               'prefix_alpha2': lambda: ops.energy_norm_prefix_fwd(clean, mask, None, P, IP, want_din=False, want_alpha2=True),
               'utterance_bwd': lambda: ops.energy_norm_bwd(clean, mask, beta2, s2u, ddin, P, IP, din=din_u),
               'prefix_bwd': lambda: ops.energy_norm_prefix_bwd(clean, mask, ratio, s2p, ddin, P, IP, din=din_p)}
        ts = {k: [] for k in fns}
        for _ in range(a.warmup):
            for k, fn in fns.items():
                _events(fn, a.inner)
        for _ in range(a.reps):                                 # the kernels alternate inside every repetition
            for k, fn in fns.items():
                ts[k].append(_events(fn, a.inner))
        row = {k: statistics.median(v) for k, v in ts.items()}
        for k in ('fwd', 'alpha2', 'bwd'):
            row['ratio_' + k] = row['prefix_' + k] / row['utterance_' + k]
        res['kernels']['B%d_T%d' % (B, T)] = row
        print('B %d T %d %s' % (B, T, json.dumps({k: round(v, 2) for k, v in row.items()})), flush=True)
    if a.step:
        B, L = 256, 64000
        c, v = synth.batch(B, L, start=0)
        cw, nw = torch.from_numpy(c).cuda(), torch.from_numpy(v).cuda()
        trs = {}
        for mode in MODES:
            trs[mode] = GanTrainer('siib&haspi&estoi', norm=mode)
            trs[mode].G.precision = trs[mode].D.precision = a.precision
        ts = {m: [] for m in MODES}
        for r in range(a.step_warmup + a.step_reps):            # the modes alternate
            for mode in MODES:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                trs[mode].canonical_step(cw, nw)
                torch.cuda.synchronize()
                if r >= a.step_warmup:
                    ts[mode].append((time.perf_counter() - t0) * 1e3)
        res['canonical_step_ms'] = {m: statistics.median(v) for m, v in ts.items()}
        res['canonical_step_ms']['spread'] = {m: [min(v), max(v)] for m, v in ts.items()}
        res['canonical_step_ms']['ratio'] = res['canonical_step_ms']['prefix'] / res['canonical_step_ms']['utterance']
        res['canonical_step_ms']['config'] = 'B = 256, L = 64000, siib&haspi&estoi, %s, wall clock with device synchronisation, %d steps after %d' % (a.precision, a.step_reps, a.step_warmup)
        print('canonical_step', json.dumps(res['canonical_step_ms']), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default='study,timing')
    ap.add_argument('--epochs', type=int, default=30)
    ap.add_argument('--utts', type=int, default=256)
    ap.add_argument('--valid', type=int, default=64)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--length', type=int, default=63871)
    ap.add_argument('--metrics', default='siib&haspi&estoi')
    ap.add_argument('--precision', default='bf16')
    ap.add_argument('--seed', type=int, default=666)
    ap.add_argument('--noise-tilt', type=float, default=1.5, help='1.5 = the low-pass-noise corpus (tools/learn_curve.py)')
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-step', dest='step', action='store_false')
    ap.add_argument('--step-reps', type=int, default=9)
    ap.add_argument('--step-warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    doc = {'tool': 'tools/prefix_norm_study.py', 'args': vars(a), 'device': torch.cuda.get_device_name(0),
           'note': 'one seed per mode: two float32 seeds of this loop end 0.013 apart in the objective (README), so the four cells are recorded, '
                   'not ranked'}
    if 'timing' in a.only.split(','):
        doc['timing'] = timing(a)
    if 'study' in a.only.split(','):
        doc['study'] = study(a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump(doc, fh, indent=1)
        print('wrote', a.out)


if __name__ == '__main__':
    main()
