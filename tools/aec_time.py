"""Per-hop device time of the echo canceller (nele_gan_amd/aec.py): python tools/aec_time.py [--hops N] [--warmup W]
[--streams 1,16,256,1024,4096] [--partitions 8,16] [--json PATH]

For every (streams, partitions): W warm-up hops, then N timed hops of one hop per call on device inputs, each between two HIP events on
the current stream, a 0.3 ms idle kernel (nele_stream_spin) queued ahead of each so that the host's enqueue never shows up as device
time.  In the same run, per streams value, RealtimeEnhancer's own hop (bf16, prefix normalisation) timed the same way: the canceller's
cost is stated against the 16 ms hop and against the enhancer it serves.  Prints one JSON line per configuration (median and p99)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nele_gan_amd import _lib, synth  # noqa: E402
from nele_gan_amd.aec import HOP, EchoCanceller  # noqa: E402
from nele_gan_amd.realtime import RealtimeEnhancer  # noqa: E402


def timed(step, hops, warmup):
    st = _lib.stream()
    ms, pend = [], []
    for i in range(warmup + hops):
        _lib.lib.nele_stream_spin(300.0, st)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step(i)
        e1.record()
        if i >= warmup:
            pend.append((e0, e1))
        if len(pend) >= 256 or i == warmup + hops - 1:      # a bounded number of live events
            torch.cuda.synchronize()
            ms.extend(x.elapsed_time(y) for x, y in pend)
            pend = []
    ms = np.array(ms)
    return float(np.median(ms)), float(np.percentile(ms, 99)), len(ms)


def device_hops(a, S):
    reps = (S + a.shape[0] - 1) // a.shape[0]
    a = np.tile(a, (reps, 1))[:S]
    return [torch.from_numpy(np.ascontiguousarray(a[:, h * HOP:(h + 1) * HOP])).cuda() for h in range(a.shape[1] // HOP)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hops', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--streams', default='1,16,256,1024,4096')
    ap.add_argument('--partitions', default='8,16')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    far, near = synth.batch(16, HOP * 100, start=900)
    rows = []
    for S in [int(s) for s in a.streams.split(',')]:
        played, noise = device_hops(far, S), device_hops(near, S)
        mic = [n + 0.5 * torch.roll(p, 40, dims=1) for n, p in zip(noise, played)]        # any signal: the work does not depend on the data
        n = len(played)
        rt = RealtimeEnhancer(streams=S, precision='bf16')
        med, p99, cnt = timed(lambda i: rt.process(played[i % n], noise[i % n]), a.hops, a.warmup)
        rt_med = med
        r = {'what': 'RealtimeEnhancer bf16', 'streams': S, 'median_ms': round(med, 4), 'p99_ms': round(p99, 4), 'hops': cnt}
        rows.append(r)
        print(json.dumps(r), flush=True)
        del rt
        for P in [int(p) for p in a.partitions.split(',')]:
            aec = EchoCanceller(S, partitions=P)
            med, p99, cnt = timed(lambda i: aec.process(mic[i % n], played[i % n]), a.hops, a.warmup)
            r = {'what': 'EchoCanceller', 'streams': S, 'partitions': P, 'median_ms': round(med, 4), 'p99_ms': round(p99, 4), 'hops': cnt,
                 'share_of_16ms_hop': round(p99 / 16.0, 4), 'against_enhancer_median': round(med / rt_med, 3)}
            rows.append(r)
            print(json.dumps(r), flush=True)
            del aec
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, 'w') as f:
            json.dump({'rows': rows}, f, indent=1)


if __name__ == '__main__':
    main()
