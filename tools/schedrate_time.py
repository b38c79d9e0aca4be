"""Per-hop device time of the scheduled stream converters (nele_gan_amd/resample.py ScheduledStreamResampler) and of
ScheduledRateEnhancer (nele_gan_amd/streamrate.py): python tools/schedrate_time.py [--hops N] [--warmup W]
[--streams 1,16,256,1024,4096] [--cases 44100:high,44100:scipy,22050:high] [--json profiles/schedrate/schedrate_time.json]

The method is tools/streamrate_time.py's (its timed() and device_hops() are used here).  For every streams value B: RealtimeEnhancer's
own hop (bf16, prefix normalisation) and RateAdaptedEnhancer at 48 kHz 'high' around it, then for every case (device rate : preset) the
down-converter (2 B slots: both signals in one launch), the up-converter (B slots) and ScheduledRateEnhancer around a bf16
RealtimeEnhancer - one hop per call on device inputs, following the schedule, so the median is over hops of both lengths.  For the
converters the rate of filter products per second (slots x mean outputs per hop x K / median); beside it, in the same process, the
offline kernel's (csrc/resample.hip) at the same ratio and preset on 256 rows of 4 s, measured as tools/resample_time.py measures it
(median of 20 calls after 3).  Prints one JSON line per configuration."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from nele_gan_amd import _lib  # noqa: E402
from nele_gan_amd.realtime import HOP, RealtimeEnhancer  # noqa: E402
from nele_gan_amd.resample import STREAM_RATE, Resampler, ScheduledStreamResampler  # noqa: E402
from nele_gan_amd.streamrate import RateAdaptedEnhancer, ScheduledRateEnhancer  # noqa: E402
from streamrate_time import device_hops, timed  # noqa: E402


def offline_rate(sr_in, sr_out, quality, rows=256, secs=4.0, reps=20):
    """products per second of one Resampler.apply call into preallocated outputs: tools/resample_time.py's measurement"""
    rs = Resampler(sr_in, sr_out, quality)
    L = int(round(secs * sr_in))
    x = torch.randn((rows, L), device='cuda', dtype=torch.float32)
    ln = torch.full((rows,), L, dtype=torch.int32, device='cuda')
    y = torch.empty((rows, rs.out_len(L)), dtype=torch.float32, device='cuda')
    no = torch.empty((rows,), dtype=torch.int32, device='cuda')
    ms = []
    for i in range(3 + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rs.apply(x, ln, out=(y, no))
        e1.record()
        e1.synchronize()
        if i >= 3:
            ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms)
    return {'what': 'Resampler offline', 'sr_in': sr_in, 'sr_out': sr_out, 'quality': quality, 'rows': rows, 'seconds': secs, 'K': rs.K,
            'median_ms': round(med, 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4),
            'products_per_s': round(float(rows) * rs.out_len(L) * rs.K / (med * 1e-3), 0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hops', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--streams', default='1,16,256,1024,4096')
    ap.add_argument('--cases', default='44100:high,44100:scipy,22050:high')
    ap.add_argument('--json', default=os.path.join('profiles', 'schedrate', 'schedrate_time.json'))
    a = ap.parse_args()
    cases = [(int(c.split(':')[0]), c.split(':')[1]) for c in a.cases.split(',')]
    rows = []

    def report(r, med=None, p99=None, cnt=None):
        if med is not None:
            r.update({'median_ms': round(med, 4), 'p99_ms': round(p99, 4), 'hops': cnt})
        rows.append(r)
        print(json.dumps(r), flush=True)

    for rate, q in cases:
        report(offline_rate(rate, STREAM_RATE, q))
        report(offline_rate(STREAM_RATE, rate, q))
    for S in [int(s) for s in a.streams.split(',')]:
        c16, n16 = device_hops(S, HOP, 8, 1), device_hops(S, HOP, 8, 2)
        rt = RealtimeEnhancer(streams=S, precision='bf16')
        rt_med, p99, cnt = timed(lambda i: rt.process(c16[i % 8], n16[i % 8]), a.hops, a.warmup)
        report({'what': 'RealtimeEnhancer bf16', 'streams': S}, rt_med, p99, cnt)
        del rt
        wrap = RateAdaptedEnhancer(RealtimeEnhancer(streams=S, precision='bf16'), 48000, 'high')
        x48 = device_hops(2 * S, wrap.hop, 8, 4)
        med, p99, cnt = timed(lambda i: wrap.process(x48[i % 8][:S], x48[i % 8][S:]), a.hops, a.warmup)
        report({'what': 'RateAdaptedEnhancer bf16', 'rate': 48000, 'quality': 'high', 'streams': S, 'latency_samples': wrap.latency,
                'share_of_16ms_hop': round(p99 / 16.0, 4), 'against_enhancer_median': round(med / rt_med, 3)}, med, p99, cnt)
        del wrap, x48
        for rate, q in cases:
            down = ScheduledStreamResampler(2 * S, rate, STREAM_RATE, q)
            P, mean = down.period, down.width_in(down.period, 0) / down.period
            xs = [device_hops(2 * S, down.width_in(1, g), 1, 3 + g)[0] for g in range(P)]       # one hop per schedule position
            med, p99, cnt = timed(lambda i: down.process(xs[down.position]), a.hops, a.warmup)
            report({'what': 'ScheduledStreamResampler down', 'rate': rate, 'quality': q, 'streams': S, 'slots': 2 * S, 'K': down.K,
                    'products_per_s': round(2 * S * HOP * down.K / (med * 1e-3), 0)}, med, p99, cnt)
            up = ScheduledStreamResampler(S, STREAM_RATE, rate, q)
            med, p99, cnt = timed(lambda i: up.process(c16[i % 8]), a.hops, a.warmup)
            report({'what': 'ScheduledStreamResampler up', 'rate': rate, 'quality': q, 'streams': S, 'slots': S, 'K': up.K,
                    'products_per_s': round(S * mean * up.K / (med * 1e-3), 0)}, med, p99, cnt)
            del down, up
            wrap = ScheduledRateEnhancer(RealtimeEnhancer(streams=S, precision='bf16'), rate, q)
            med, p99, cnt = timed(lambda i: wrap.process(xs[wrap.down.position][:S], xs[wrap.down.position][S:]), a.hops, a.warmup)
            report({'what': 'ScheduledRateEnhancer bf16', 'rate': rate, 'quality': q, 'streams': S, 'latency_samples': float(wrap.latency),
                    'share_of_16ms_hop': round(p99 / 16.0, 4), 'against_enhancer_median': round(med / rt_med, 3)}, med, p99, cnt)
            del wrap, xs
            torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump({'device': _lib.device_info(), 'rows': rows}, f, indent=1)


if __name__ == '__main__':
    main()
