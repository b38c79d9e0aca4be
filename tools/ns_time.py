"""Per-hop device time of the noise suppressor (nele_gan_amd/ns.py): python tools/ns_time.py [--hops N] [--warmup W]
[--streams 1,16,256,1024,4096] [--json PATH]

For every streams value: W warm-up hops, then N timed hops of one hop per call on device inputs, each between two HIP events on the
current stream, a 0.3 ms idle kernel (nele_stream_spin) queued ahead of each so that the host's enqueue never shows up as device time
(tools/aec_time.py's method, its timed() and inputs).  The warm-up is at least 20 hops, so that every timed hop runs the whole IMCRA
frame (from frame 15 on) and every 15th of them the minima store.  In the same run, per streams value, the ResidualEchoSuppressor of
DESIGN.md section 17, timed the same way, and the NoiseSuppressor with its three optional outputs.  Prints one JSON line per
configuration (median and p99)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from aec_time import device_hops, timed  # noqa: E402
from nele_gan_amd import _lib, synth  # noqa: E402
from nele_gan_amd.ns import HOP, WANT, NoiseSuppressor  # noqa: E402
from nele_gan_amd.res import ResidualEchoSuppressor  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hops', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--streams', default='1,16,256,1024,4096')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    warmup = max(a.warmup, 20)
    far, near = synth.batch(16, HOP * 100, start=900)
    rec = int(_lib.lib.nele_ns_stream_record_bytes())
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
        mix = [s + n for s, n in zip(speech, noise)]                # speech in noise: E1's iteration counts depend on the SNRs
        n = len(mix)
        res = ResidualEchoSuppressor(S)
        base = row('ResidualEchoSuppressor', S, timed(lambda i: res.process(noise[i % n], speech[i % n]), a.hops, warmup))
        ns = NoiseSuppressor(S)
        alone = row('NoiseSuppressor', S, timed(lambda i: ns.process(mix[i % n]), a.hops, warmup), record_bytes=rec)
        alone['against_res_median'] = round(alone['median_ms'] / base['median_ms'], 3)
        full = NoiseSuppressor(S)
        bufs = (torch.empty((S, HOP), device='cuda'),) + tuple(torch.empty((S, 1, 257), dtype=torch.float64, device='cuda') for _ in WANT)
        row('NoiseSuppressor + gains, noise_psd, presence', S, timed(lambda i: full.process(mix[i % n], want=WANT, out=bufs), a.hops, warmup))
        del res, ns, full
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, 'w') as f:
            json.dump({'rows': rows}, f, indent=1)


if __name__ == '__main__':
    main()
