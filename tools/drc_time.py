"""Per-hop device time of the stream compressor (nele_gan_amd/drc.py): python tools/drc_time.py [--hops N] [--warmup W]
[--streams 1,16,256,1024,4096] [--json PATH]

For every streams value: W warm-up hops, then N timed hops of one hop per call on device inputs, each between two HIP events on the
current stream, a 0.3 ms idle kernel (nele_stream_spin) queued ahead of each so that the host's enqueue never shows up as device time
(tools/aec_time.py's method, its timed() and inputs).  The work of a hop does not depend on the data: 416 magnitudes, 256 means, 256
dependent attack / release steps.  In the same run, per streams value, the ResidualEchoSuppressor of DESIGN.md section 17 and the
rule-mode RealtimeEnhancer of section 22 - the stage the compressor stands behind - timed the same way, the compressor with its two
optional outputs, and the two stages chained (CompressedEnhancer).  Prints one JSON line per configuration (median and p99)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from aec_time import device_hops, timed  # noqa: E402
from nele_gan_amd import _lib, synth  # noqa: E402
from nele_gan_amd.drc import HOP, CompressedEnhancer, StreamCompressor  # noqa: E402
from nele_gan_amd.realtime import RealtimeEnhancer  # noqa: E402
from nele_gan_amd.res import ResidualEchoSuppressor  # noqa: E402
from nele_gan_amd.siiopt import SiiOptRule  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hops', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--streams', default='1,16,256,1024,4096')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    far, near = synth.batch(16, HOP * 100, start=900)
    rec = int(_lib.lib.nele_drc_stream_record_bytes())
    rows = []

    def row(what, S, stats, **more):
        med, p99, cnt = stats
        r = dict({'what': what, 'streams': S, 'median_ms': round(med, 4), 'p99_ms': round(p99, 4), 'hops': cnt,
                  'share_of_16ms_hop': round(p99 / 16.0, 5)}, **more)
        rows.append(r)
        print(json.dumps(r), flush=True)
        return r

    for S in [int(s) for s in a.streams.split(',')]:
        speech, noise = device_hops(far, S), device_hops(near, S)
        n = len(speech)
        res = ResidualEchoSuppressor(S)
        row('ResidualEchoSuppressor', S, timed(lambda i: res.process(noise[i % n], speech[i % n]), a.hops, a.warmup))
        rt = RealtimeEnhancer(rule=SiiOptRule(), streams=S)
        rule = row('RealtimeEnhancer rule', S, timed(lambda i: rt.process(speech[i % n], noise[i % n]), a.hops, a.warmup))
        drc = StreamCompressor(S)
        alone = row('StreamCompressor', S, timed(lambda i: drc.process(speech[i % n]), a.hops, a.warmup), record_bytes=rec)
        alone['against_rule_median'] = round(alone['median_ms'] / rule['median_ms'], 3)
        full = StreamCompressor(S)
        bufs = (torch.empty((S, HOP), device='cuda'), torch.empty((S, HOP), dtype=torch.float64, device='cuda'),
                torch.empty((S, 1), dtype=torch.float64, device='cuda'))
        row('StreamCompressor + gain, level', S, timed(lambda i: full.process(speech[i % n], want=('gain', 'level'), out=bufs), a.hops, a.warmup))
        chain = CompressedEnhancer(RealtimeEnhancer(rule=SiiOptRule(), streams=S), StreamCompressor(S))
        row('CompressedEnhancer rule', S, timed(lambda i: chain.process(speech[i % n], noise[i % n]), a.hops, a.warmup))
        del res, rt, drc, full, chain
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, 'w') as f:
            json.dump({'rows': rows}, f, indent=1)


if __name__ == '__main__':
    main()
