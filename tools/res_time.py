"""Per-hop device time of the residual-echo suppressor (nele_gan_amd/res.py): python tools/res_time.py [--hops N] [--warmup W]
[--streams 1,16,256,1024,4096] [--partitions 8] [--json PATH]

For every streams value: W warm-up hops, then N timed hops of one hop per call on device inputs, each between two HIP events on the
current stream, a 0.3 ms idle kernel (nele_stream_spin) queued ahead of each so that the host's enqueue never shows up as device time
(tools/aec_time.py's method, its timed() and inputs).  In the same run, per streams value, the EchoCanceller it stands behind, timed
the same way, and the two chained as SuppressedEchoCanceller runs them.  Prints one JSON line per configuration (median and p99)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from aec_time import device_hops, timed  # noqa: E402
from nele_gan_amd import synth  # noqa: E402
from nele_gan_amd.aec import HOP, EchoCanceller  # noqa: E402
from nele_gan_amd.res import ResidualEchoSuppressor, SuppressedEchoCanceller  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hops', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--streams', default='1,16,256,1024,4096')
    ap.add_argument('--partitions', type=int, default=8)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    far, near = synth.batch(16, HOP * 100, start=900)
    rows = []

    def row(what, S, stats, **more):
        med, p99, cnt = stats
        r = dict({'what': what, 'streams': S, 'median_ms': round(med, 4), 'p99_ms': round(p99, 4), 'hops': cnt,
                  'share_of_16ms_hop': round(p99 / 16.0, 5)}, **more)
        rows.append(r)
        print(json.dumps(r), flush=True)
        return r

    for S in [int(s) for s in a.streams.split(',')]:
        played, noise = device_hops(far, S), device_hops(near, S)
        mic = [n + 0.5 * torch.roll(p, 40, dims=1) for n, p in zip(noise, played)]        # any signal: the work does not depend on the data
        n = len(played)
        aec = EchoCanceller(S, partitions=a.partitions)
        base = row('EchoCanceller', S, timed(lambda i: aec.process(mic[i % n], played[i % n]), a.hops, a.warmup), partitions=a.partitions)
        res = ResidualEchoSuppressor(S)
        # the suppressor alone, on residual-like and echo-like inputs already on the device
        alone = row('ResidualEchoSuppressor', S, timed(lambda i: res.process(noise[i % n], played[i % n]), a.hops, a.warmup))
        alone['against_canceller_median'] = round(alone['median_ms'] / base['median_ms'], 3)
        both = SuppressedEchoCanceller(aec, res)
        row('SuppressedEchoCanceller', S, timed(lambda i: both.process(mic[i % n], played[i % n]), a.hops, a.warmup), partitions=a.partitions)
        del aec, res, both
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, 'w') as f:
            json.dump({'rows': rows}, f, indent=1)


if __name__ == '__main__':
    main()
