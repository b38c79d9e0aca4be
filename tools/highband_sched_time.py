"""Per-hop device time of the scheduled up-converter that carries the high band (nele_gan_amd/highband.py ScheduledHighBandUp,
csrc/highband_sched.hip) beside the plain scheduled one: python tools/highband_sched_time.py [--hops N] [--warmup W]
[--streams 1,16,256,1024,4096] [--rate 44100] [--quality high] [--out profiles/highband_sched/highband_sched_time.txt]

For every streams value B, in one run: the plain 16 kHz -> device-rate ScheduledStreamResampler launch, the fused ScheduledHighBandUp
launch, and ScheduledRateEnhancer beside FullBandScheduledEnhancer around a bf16 RealtimeEnhancer.  The protocol is DESIGN section
20's (tools/streamrate_time.py's timed() and device_hops()): W warm-up hops, then N timed hops of one hop per call on device inputs
following the schedule - so the median is over hops of both lengths -, each between two HIP events on the current stream, a 0.3 ms
idle kernel queued ahead of each so that the host's enqueue never shows up as device time.  One JSON line per configuration (median
and p99).  Beside the fused launch's: the bytes per stream and hop it moves beyond the plain launch's, counted from the record layouts
- the x row and the low row read, the record of H + lag16 + lag floats read and written in place of the converter's H."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from nele_gan_amd.highband import ScheduledHighBandUp  # noqa: E402
from nele_gan_amd.realtime import HOP, RealtimeEnhancer  # noqa: E402
from nele_gan_amd.resample import STREAM_RATE, ScheduledStreamResampler  # noqa: E402
from nele_gan_amd.streamrate import FullBandScheduledEnhancer, ScheduledRateEnhancer  # noqa: E402
from streamrate_time import device_hops, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hops', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--streams', default='1,16,256,1024,4096')
    ap.add_argument('--rate', type=int, default=44100)
    ap.add_argument('--quality', default='high')
    ap.add_argument('--out', default=os.path.join('profiles', 'highband_sched', 'highband_sched_time.txt'))
    a = ap.parse_args()
    lines, NSIG = [], 8

    def report(r, med, p99, cnt):
        r.update({'median_ms': round(med, 4), 'p99_ms': round(p99, 4), 'hops': cnt})
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)

    for S in [int(s) for s in a.streams.split(',')]:
        up = ScheduledStreamResampler(S, STREAM_RATE, a.rate, a.quality)
        hb = ScheduledHighBandUp(S, a.rate, 1, a.quality)
        P, mean = hb.period, hb.width_out(hb.period, 0) / hb.period
        e16, l16 = device_hops(S, HOP, NSIG, 1), device_hops(S, HOP, NSIG, 2)
        xs = [device_hops(2 * S, hb.width_out(1, g), 1, 3 + g)[0] for g in range(P)]           # one hop per schedule position
        outs = [torch.empty((S, hb.width_out(1, g)), dtype=torch.float32, device='cuda') for g in range(P)]
        base = {'rate': a.rate, 'quality': a.quality, 'streams': S, 'K': hb.K, 'table_bytes': 8 * hb.up * hb.K}
        up_med, p99, cnt = timed(lambda i: up.process(e16[i % NSIG], out=outs[up.position]), a.hops, a.warmup)
        own = 4 * (HOP + mean + 2 * up.H)                   # the plain launch's bytes per stream and hop
        report(dict(base, what='ScheduledStreamResampler up', bytes_per_stream=round(own, 1), gb_per_s=round(S * own / (up_med * 1e-3) / 1e9, 1)),
               up_med, p99, cnt)
        extra = 4 * (mean + HOP + 2 * (hb.H + hb.lag16 + hb.lag)) - 4 * 2 * up.H
        med, p99, cnt = timed(lambda i: hb.process(e16[i % NSIG], l16[i % NSIG], xs[hb.position][:S], out=outs[hb.position]), a.hops, a.warmup)
        report(dict(base, what='ScheduledHighBandUp', shift=hb.shift, lag16=hb.lag16, lag=hb.lag, extra_bytes_per_stream=round(extra, 1),
                    against_up_median=round(med / up_med, 3), over_up_ms=round(med - up_med, 4)), med, p99, cnt)
        del up, hb, e16, l16, outs
        meds = {}
        for cls in (ScheduledRateEnhancer, FullBandScheduledEnhancer):
            wrap = cls(RealtimeEnhancer(streams=S, precision='bf16'), a.rate, a.quality)
            meds[cls], p99, cnt = timed(lambda i: wrap.process(xs[wrap.down.position][:S], xs[wrap.down.position][S:]), a.hops, a.warmup)
            r = dict(base, what=cls.__name__ + ' bf16', latency_samples=float(wrap.latency), share_of_16ms_hop=round(p99 / 16.0, 4))
            if cls is FullBandScheduledEnhancer:
                r['against_plain_median'] = round(meds[cls] / meds[ScheduledRateEnhancer], 4)
            report(r, meds[cls], p99, cnt)
            del wrap
        del xs
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
