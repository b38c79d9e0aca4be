#!/usr/bin/env python
"""Device time of the partitioned FFT convolution (nele_fir_fft_var) against the direct filter (nele_fir_filter) in one process, and one
canonical step with and without a room.

    python tools/room_time.py [--out profiles/room/room_time.json] [--no-step]

Filters: B = 256 with (L, Lh) = (64000, 16000) and (63871, 9001); HIP events around one call, 3 warm-up calls, median of 20, the two
calls timed in alternating blocks (a b a b) so that clock drift meets both.  `ratio` = direct median / FFT median; the run fails
(exit 1) when it is below 10 at (64000, 16000) - 2 L Lh = 2.05 GFLOP per row against about 44 MFLOP, a ratio of 46 in arithmetic.
Step: GanTrainer('siib&haspi&estoi').canonical_step at B = 256, L = 64000 (BASELINE configs[2]) with room=None and with a bank of two
1 s RIRs (rows alternate), wall time per step over 10 steps after 3, synchronised at both ends."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dev_ms(fn, reps=10, warm=3):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def rir(n, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    h = rng.standard_normal(n) * np.exp(-np.arange(n) / (n / 7.0)) * 0.2
    h[37] = 1.0
    return h.astype(np.float32)


def filters():
    import numpy as np
    import torch
    from nele_gan_amd import eval_metrics, room
    from nele_gan_amd._lib import call, ptr, stream
    out = {}
    for B, L, Lh in ((256, 64000, 16000), (256, 63871, 9001)):
        rng = np.random.default_rng(L)
        x = torch.from_numpy(rng.standard_normal((B, L)).astype(np.float32)).cuda()
        h = rir(Lh, 3).astype(np.float64)
        hd = torch.from_numpy(h).cuda()
        bank = room.prepare_bank([h])
        ws = torch.empty(room._bytes('nele_fir_fft_workspace_bytes', B, L), dtype=torch.uint8, device='cuda')
        y1, y2 = torch.empty((B, L), dtype=torch.float64, device='cuda'), torch.empty((B, L), dtype=torch.float64, device='cuda')
        fft = lambda: call('nele_fir_fft_var', ptr(x), B, L, None, ptr(bank), None, ptr(y1), ptr(ws), stream())
        direct = lambda: call('nele_fir_filter', ptr(x), B, L, ptr(hd), Lh, ptr(y2), stream())
        t_f, t_d = [], []
        for _ in range(2):
            t_f += dev_ms(fft)
            t_d += dev_ms(direct)
        err = float((y1 - y2).abs().max() / y2.abs().max())
        r = {'fft_ms': statistics.median(t_f), 'fft_min_ms': min(t_f), 'fft_max_ms': max(t_f), 'direct_ms': statistics.median(t_d),
             'direct_min_ms': min(t_d), 'direct_max_ms': max(t_d), 'reps': len(t_f), 'max_rel_diff': err,
             'workspace_bytes': int(ws.numel())}
        r['ratio'] = r['direct_ms'] / r['fft_ms']
        out['B=%d L=%d Lh=%d' % (B, L, Lh)] = r
        print(B, L, Lh, {k: (round(v, 4) if isinstance(v, float) and v > 1e-6 else v) for k, v in r.items()}, flush=True)
    return out


def steps(B=256, L=64000, n=10, warm=3):
    import numpy as np
    import torch
    from nele_gan_amd import room, synth
    from nele_gan_amd.train_nele import GanTrainer
    c, v = synth.batch(8, L, start=500)
    cw = torch.from_numpy(np.ascontiguousarray(c[np.arange(B) % 8])).cuda()
    nw = torch.from_numpy(np.ascontiguousarray(v[np.arange(B) % 8])).cuda()
    ids = (np.arange(B) % 2).astype(np.int32)
    out = {}
    for tag in ('no room', 'room', 'no room (again)', 'room (again)'):
        bank = room.RirBank({'a': rir(16000, 1), 'b': rir(16000, 2)}) if tag.startswith('room') else None
        tr = GanTrainer('siib&haspi&estoi', room=bank)
        kw = {'rir_ids': ids} if bank is not None else {}
        ts = []
        for k in range(warm + n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.canonical_step(cw, nw, **kw)
            tr.flush()
            torch.cuda.synchronize()
            if k >= warm:
                ts.append((time.perf_counter() - t0) * 1e3)
        st = tr.check_status(raise_on_error=False)
        out[tag] = {'median_ms': statistics.median(ts), 'min_ms': min(ts), 'max_ms': max(ts), 'steps': n, 'status': st}
        print(tag, out[tag], flush=True)
        del tr
        torch.cuda.empty_cache()
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'room', 'room_time.json'))
    ap.add_argument('--no-step', action='store_true')
    a = ap.parse_args()
    res = {'filters': filters()}
    if not a.no_step:
        res['canonical_step B=256 L=64000 siib&haspi&estoi'] = steps()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    ratio = res['filters']['B=256 L=64000 Lh=16000']['ratio']
    print('ratio at L=64000 Lh=16000: %.1f' % ratio)
    sys.exit(0 if ratio >= 10 else 1)
