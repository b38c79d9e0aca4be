#!/usr/bin/env python
"""Device time of the polyphase resampler (csrc/resample.hip) at 256 x 4 s from 48, 44.1, 22.05 and 8 kHz to 16 kHz and 128 x 8 s from
48 kHz, both filter presets, beside scipy.signal.resample_poly on 16 host threads for the same batch.

    python tools/resample_time.py [--out profiles/resample/resample_time.json] [--no-scipy]

Device: HIP events around one Resampler.apply call into preallocated outputs, median of 20 after 3 warm-up calls.  Per shape the time,
the float64 products per second (n_out K per row: what the kernel executes, padded taps included) and the bytes per second (float32
rows in and out, once each; the table is re-read from cache and not counted).  Host: resample_poly on the float32 rows with the library's
taps, rows dealt to 16 threads, one pass, wall clock."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(256, 4.0, sr) for sr in (48000, 44100, 22050, 8000)] + [(128, 8.0, 48000)]


def main():
    import numpy as np
    import torch
    from nele_gan_amd import _lib, resample
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'resample', 'resample_time.json'))
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--no-scipy', action='store_true')
    a = ap.parse_args()
    res = {'device': _lib.device_info(), 'reps': a.reps, 'tile': resample.TILE, 'shapes': {}}
    gen = torch.Generator(device='cuda').manual_seed(1)
    for B, secs, sr in SHAPES:
        L = int(round(secs * sr))
        x = torch.randn((B, L), generator=gen, device='cuda', dtype=torch.float32)
        lens = np.full(B, L, dtype=np.int32)
        ln = torch.from_numpy(lens).cuda()
        x_host = None if a.no_scipy else x.cpu().numpy()
        for preset in ('high', 'scipy'):
            rs = resample.Resampler(sr, 16000, preset)
            n_out = rs.out_len(L)
            y = torch.empty((B, n_out), dtype=torch.float32, device='cuda')
            no = torch.empty((B,), dtype=torch.int32, device='cuda')
            for _ in range(3):
                rs.apply(x, ln, out=(y, no))
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rs.apply(x, ln, out=(y, no))
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            med = statistics.median(ms)
            products, nbytes = float(B) * n_out * rs.K, 4.0 * B * (L + n_out)
            r = {'up': rs.up, 'down': rs.down, 'K': rs.K, 'table_KiB': rs.up * rs.K * 8 / 1024.0, 'n_out': n_out, 'median_ms': med, 'min_ms': min(ms),
                 'max_ms': max(ms), 'products_per_s': products / (med * 1e-3), 'bytes_per_s': nbytes / (med * 1e-3), 'seconds_of_audio': B * secs}
            if x_host is not None:
                from concurrent.futures import ThreadPoolExecutor
                from scipy.signal import resample_poly
                win = resample.taps(rs.up, rs.down, rs.zeros, rs.beta) / rs.up
                t0 = time.perf_counter()
                with ThreadPoolExecutor(16) as pool:
                    out = list(pool.map(lambda row: resample_poly(row, rs.up, rs.down, window=win), x_host))
                r['scipy_16_threads_ms'] = (time.perf_counter() - t0) * 1e3
                r['max_abs_difference_from_scipy'] = float(np.abs(np.stack(out) - y.cpu().numpy()).max())
            res['shapes']['%d x %g s, %d Hz, %s' % (B, secs, sr, preset)] = r
            print(B, secs, sr, preset, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
