"""Per-hop device time of the stream converters (nele_gan_amd/resample.py StreamResampler) and of RateAdaptedEnhancer
(nele_gan_amd/streamrate.py): python tools/streamrate_time.py [--hops N] [--warmup W] [--streams 1,16,256,1024,4096]
[--rates 48000,8000] [--qualities high,scipy] [--json profiles/streamrate/streamrate_time.json]

For every streams value B: RealtimeEnhancer's own hop (bf16, prefix normalisation), then for every device rate and preset the
down-converter (2 B slots: both signals in one launch), the up-converter (B slots) and RateAdaptedEnhancer around a bf16
RealtimeEnhancer.  W warm-up hops, then N timed hops of one hop per call on device inputs, each between two HIP events on the current
stream, a 0.3 ms idle kernel (nele_stream_spin) queued ahead of each so that the host's enqueue never shows up as device time (as
tools/aec_time.py).  Prints one JSON line per configuration (median and p99; for the converters the rate of filter products per second,
slots x outputs x K / median, to set beside the offline kernel's in profiles/resample/resample_time.json)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nele_gan_amd import _lib  # noqa: E402
from nele_gan_amd.realtime import HOP, RealtimeEnhancer  # noqa: E402
from nele_gan_amd.resample import STREAM_RATE, StreamResampler  # noqa: E402
from nele_gan_amd.streamrate import RateAdaptedEnhancer  # noqa: E402


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


def device_hops(rows, width, n, seed):
    """n different hops [rows, width] of Gaussian samples on the device (any signal: the work does not depend on the data)"""
    g = torch.Generator(device='cuda').manual_seed(seed)
    return [0.1 * torch.randn((rows, width), device='cuda', generator=g) for _ in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hops', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--streams', default='1,16,256,1024,4096')
    ap.add_argument('--rates', default='48000,8000')
    ap.add_argument('--qualities', default='high,scipy')
    ap.add_argument('--json', default=os.path.join('profiles', 'streamrate', 'streamrate_time.json'))
    a = ap.parse_args()
    rows, NSIG = [], 8

    def report(r, med, p99, cnt):
        r.update({'median_ms': round(med, 4), 'p99_ms': round(p99, 4), 'hops': cnt})
        rows.append(r)
        print(json.dumps(r), flush=True)

    for S in [int(s) for s in a.streams.split(',')]:
        c16, n16 = device_hops(S, HOP, NSIG, 1), device_hops(S, HOP, NSIG, 2)
        rt = RealtimeEnhancer(streams=S, precision='bf16')
        rt_med, p99, cnt = timed(lambda i: rt.process(c16[i % NSIG], n16[i % NSIG]), a.hops, a.warmup)
        report({'what': 'RealtimeEnhancer bf16', 'streams': S}, rt_med, p99, cnt)
        del rt
        for rate in [int(r) for r in a.rates.split(',')]:
            for q in a.qualities.split(','):
                down = StreamResampler(2 * S, rate, STREAM_RATE, q)
                xs = device_hops(2 * S, down.hop_in, NSIG, 3)
                med, p99, cnt = timed(lambda i: down.process(xs[i % NSIG]), a.hops, a.warmup)
                report({'what': 'StreamResampler down', 'rate': rate, 'quality': q, 'streams': S, 'slots': 2 * S, 'K': down.K,
                        'products_per_s': round(2 * S * down.hop_out * down.K / (med * 1e-3), 0)}, med, p99, cnt)
                up = StreamResampler(S, STREAM_RATE, rate, q)
                med, p99, cnt = timed(lambda i: up.process(c16[i % NSIG]), a.hops, a.warmup)
                report({'what': 'StreamResampler up', 'rate': rate, 'quality': q, 'streams': S, 'slots': S, 'K': up.K,
                        'products_per_s': round(S * up.hop_out * up.K / (med * 1e-3), 0)}, med, p99, cnt)
                hop = down.hop_in
                del down, up
                wrap = RateAdaptedEnhancer(RealtimeEnhancer(streams=S, precision='bf16'), rate, q)
                med, p99, cnt = timed(lambda i: wrap.process(xs[i % NSIG][:S], xs[i % NSIG][S:]), a.hops, a.warmup)
                report({'what': 'RateAdaptedEnhancer bf16', 'rate': rate, 'quality': q, 'streams': S, 'latency_samples': wrap.latency,
                        'share_of_16ms_hop': round(p99 / 16.0, 4), 'against_enhancer_median': round(med / rt_med, 3)}, med, p99, cnt)
                del wrap, xs
                torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump({'rows': rows}, f, indent=1)


if __name__ == '__main__':
    main()
