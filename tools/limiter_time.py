"""Per-hop device time of the stream limiter (nele_gan_amd/limiter.py): python tools/limiter_time.py [--hops N] [--warmup W]
[--streams 1,16,256,1024,4096] [--only-limiter] [--tag NAME] [--json PATH]

For every streams value: W warm-up hops, then N timed hops of one hop per call on device inputs, each between two HIP events on the
current stream, a 0.3 ms idle kernel (nele_stream_spin) queued ahead of each so that the host's enqueue never shows up as device time
(tools/drc_time.py's method, tools/aec_time.py's timed() and inputs).  The work of a hop does not depend on the data: 256 + LA peaks of
three 12-tap sums, 256 minima and 256 means of LA + 1 terms, 256 dependent steps of the decaying maximum.  In the same run, per streams
value, the StreamCompressor of DESIGN.md section 23 and the rule-mode RealtimeEnhancer of section 22, the limiter with its two optional
outputs, on sample peaks only, at LA = 192, chained behind the compressor, and the whole chain LimitedEnhancer(CompressedEnhancer).
--only-limiter: the limiter's own rows alone (for timing-only builds loaded through NELE_LIB; --tag names the build in every row).
Prints one JSON line per configuration (median and p99)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from aec_time import device_hops, timed  # noqa: E402
from nele_gan_amd import _lib, synth  # noqa: E402
from nele_gan_amd.drc import CompressedEnhancer, StreamCompressor  # noqa: E402
from nele_gan_amd.limiter import HOP, LimitedEnhancer, StreamLimiter  # noqa: E402
from nele_gan_amd.realtime import RealtimeEnhancer  # noqa: E402
from nele_gan_amd.siiopt import SiiOptRule  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hops', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--streams', default='1,16,256,1024,4096')
    ap.add_argument('--only-limiter', action='store_true')
    ap.add_argument('--tag', default=None)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    far, near = synth.batch(16, HOP * 100, start=900)
    far = far * 8.0                                        # loud enough for the limiter to act (its work does not depend on it)
    rows = []

    def row(what, S, stats, **more):
        med, p99, cnt = stats
        r = dict({'what': what, 'streams': S, 'median_ms': round(med, 4), 'p99_ms': round(p99, 4), 'hops': cnt,
                  'share_of_16ms_hop': round(p99 / 16.0, 5)}, **more)
        if a.tag:
            r['lib'] = a.tag
        rows.append(r)
        print(json.dumps(r), flush=True)
        return r

    for S in [int(s) for s in a.streams.split(',')]:
        speech, noise = device_hops(far, S), device_hops(near, S)
        n = len(speech)
        lim = StreamLimiter(S)
        rec = int(_lib.lib.nele_lim_stream_record_bytes(lim.lookahead))
        alone = row('StreamLimiter', S, timed(lambda i: lim.process(speech[i % n]), a.hops, a.warmup), record_bytes=rec)
        if not a.only_limiter:
            drc = StreamCompressor(S)
            comp = row('StreamCompressor', S, timed(lambda i: drc.process(speech[i % n]), a.hops, a.warmup))
            alone['against_compressor_median'] = round(alone['median_ms'] / comp['median_ms'], 3)
            rt = RealtimeEnhancer(rule=SiiOptRule(), streams=S)
            row('RealtimeEnhancer rule', S, timed(lambda i: rt.process(speech[i % n], noise[i % n]), a.hops, a.warmup))
            full = StreamLimiter(S)
            bufs = (torch.empty((S, HOP), device='cuda'), torch.empty((S, HOP), dtype=torch.float64, device='cuda'),
                    torch.empty((S, 1), dtype=torch.float64, device='cuda'))
            row('StreamLimiter + gain, peak', S, timed(lambda i: full.process(speech[i % n], want=('gain', 'peak'), out=bufs), a.hops, a.warmup))
            drc2, lim2 = StreamCompressor(S), StreamLimiter(S)
            row('StreamCompressor, StreamLimiter chained', S, timed(lambda i: lim2.process(drc2.process(speech[i % n])), a.hops, a.warmup))
            chain = LimitedEnhancer(CompressedEnhancer(RealtimeEnhancer(rule=SiiOptRule(), streams=S), StreamCompressor(S)), StreamLimiter(S))
            row('LimitedEnhancer(CompressedEnhancer rule)', S, timed(lambda i: chain.process(speech[i % n], noise[i % n]), a.hops, a.warmup))
            del drc, rt, full, drc2, lim2, chain
        plain = StreamLimiter(S, true_peak=False)
        row('StreamLimiter sample peaks', S, timed(lambda i: plain.process(speech[i % n]), a.hops, a.warmup))
        wide = StreamLimiter(S, lookahead=192)
        row('StreamLimiter LA 192', S, timed(lambda i: wide.process(speech[i % n]), a.hops, a.warmup))
        del lim, plain, wide
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, 'w') as f:
            json.dump({'rows': rows}, f, indent=1)


if __name__ == '__main__':
    main()
