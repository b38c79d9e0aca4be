"""Per-hop device time of the up-converter that carries the high band (nele_gan_amd/highband.py HighBandUp, csrc/highband.hip) beside
the plain one: python tools/highband_time.py [--hops N] [--warmup W] [--streams 1,16,256,1024,4096] [--rate 48000] [--quality high]
[--out profiles/highband/highband_time.txt]

For every streams value B, in one run: the plain 16 kHz -> device-rate StreamResampler launch, the fused HighBandUp launch, and
RateAdaptedEnhancer around a bf16 RealtimeEnhancer without and with ``highband``.  The protocol is tools/streamrate_time.py's: W
warm-up hops, then N timed hops of one hop per call on device inputs, each between two HIP events on the current stream, a 0.3 ms idle
kernel queued ahead of each so that the host's enqueue never shows up as device time.  One JSON line per configuration (median and
p99).  Beside the fused launch's: the bytes per stream and hop it moves beyond the plain launch's, counted from the record layout -
the x row and the low row read, the record of K - 1 + lag16 + lag floats read and written in place of the converter's K - 1 - and the
time those bytes take at the bandwidth the plain launch reaches in the same run (its own bytes: the enh row, the output row and its
record read and written, over its median)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nele_gan_amd.highband import HighBandUp  # noqa: E402
from nele_gan_amd.realtime import HOP, RealtimeEnhancer  # noqa: E402
from nele_gan_amd.resample import STREAM_RATE, StreamResampler  # noqa: E402
from nele_gan_amd.streamrate import RateAdaptedEnhancer  # noqa: E402
from streamrate_time import device_hops, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hops', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--streams', default='1,16,256,1024,4096')
    ap.add_argument('--rate', type=int, default=48000)
    ap.add_argument('--quality', default='high')
    ap.add_argument('--out', default=os.path.join('profiles', 'highband', 'highband_time.txt'))
    a = ap.parse_args()
    lines, NSIG = [], 8

    def report(r, med, p99, cnt):
        r.update({'median_ms': round(med, 4), 'p99_ms': round(p99, 4), 'hops': cnt})
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)

    for S in [int(s) for s in a.streams.split(',')]:
        up = StreamResampler(S, STREAM_RATE, a.rate, a.quality)
        hb = HighBandUp(S, a.rate, 1, a.quality)
        N = hb.hop_out
        e16, l16, x = device_hops(S, HOP, NSIG, 1), device_hops(S, HOP, NSIG, 2), device_hops(S, N, NSIG, 3)
        out = torch.empty((S, N), dtype=torch.float32, device='cuda')
        base = {'rate': a.rate, 'quality': a.quality, 'streams': S, 'K': hb.K}
        up_med, p99, cnt = timed(lambda i: up.process(e16[i % NSIG], out=out), a.hops, a.warmup)
        own = 4 * (HOP + N + 2 * (up.K - 1))                # the plain launch's bytes per stream and hop
        gbs = S * own / (up_med * 1e-3) / 1e9
        report(dict(base, what='StreamResampler up', bytes_per_stream=own, gb_per_s=round(gbs, 1)), up_med, p99, cnt)
        extra = 4 * (N + HOP + 2 * (hb.K - 1 + hb.lag16 + hb.lag)) - 4 * 2 * (up.K - 1)
        med, p99, cnt = timed(lambda i: hb.process(e16[i % NSIG], l16[i % NSIG], x[i % NSIG], out=out), a.hops, a.warmup)
        report(dict(base, what='HighBandUp', lag16=hb.lag16, lag=hb.lag, extra_bytes_per_stream=extra, against_up_median=round(med / up_med, 3),
                    extra_ms_at_up_bandwidth=round(S * extra / (gbs * 1e9) * 1e3, 4), over_up_ms=round(med - up_med, 4)), med, p99, cnt)
        del up, hb, e16, l16, out
        xs = device_hops(2 * S, N, NSIG, 4)
        meds = {}
        for key in (None, True):
            wrap = RateAdaptedEnhancer(RealtimeEnhancer(streams=S, precision='bf16'), a.rate, a.quality, highband=key)
            meds[key], p99, cnt = timed(lambda i: wrap.process(xs[i % NSIG][:S], xs[i % NSIG][S:]), a.hops, a.warmup)
            r = dict(base, what='RateAdaptedEnhancer bf16', highband=key, latency_samples=wrap.latency, share_of_16ms_hop=round(p99 / 16.0, 4))
            if key:
                r['against_plain_median'] = round(meds[True] / meds[None], 4)
            report(r, meds[key], p99, cnt)
            del wrap
        del xs, x
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
