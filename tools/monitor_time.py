"""Per-hop device time of the running ESTOI (nele_gan_amd/monitor.py): python tools/monitor_time.py [--hops N] [--warmup W]
[--streams 1,16,256,1024,4096] [--json PATH]

For every streams value: W warm-up hops, then N timed hops of one hop per call on device inputs, each between two HIP events on the
current stream, a 0.3 ms idle kernel (nele_stream_spin) queued ahead of each so that the host's enqueue never shows up as device time
(tools/aec_time.py's method, its timed() and inputs; tools/ns_time.py's frame).  The warm-up is at least 50 hops, so that every timed
hop completes one or two frames, re-analyses them and forms their segments (the ring holds 30 band vectors from hop 26 on).  In the
same run, per streams value, the NoiseSuppressor's hop, timed the same way, then the monitor with ref, deg and add at lag 1, with its
three optional outputs, and as MonitoredEnhancer's pair (the processed signal and the baseline).  Prints one JSON line per
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
from nele_gan_amd.monitor import HOP, WANT, StreamMonitor  # noqa: E402
from nele_gan_amd.ns import NoiseSuppressor  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hops', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--streams', default='1,16,256,1024,4096')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    warmup = max(a.warmup, 50)
    far, near = synth.batch(16, HOP * 100, start=900)
    rec = int(_lib.lib.nele_mon_stream_record_bytes())
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
        mix = [s + n for s, n in zip(speech, noise)]
        n = len(mix)
        ns = NoiseSuppressor(S)
        base = row('NoiseSuppressor', S, timed(lambda i: ns.process(mix[i % n]), a.hops, warmup))
        del ns
        mon = StreamMonitor(S, lag=1)
        alone = row('StreamMonitor', S, timed(lambda i: mon.process(speech[i % n], speech[(i - 1) % n], noise[i % n]), a.hops, warmup),
                    record_bytes=rec, state_traffic_mb=round(2e-6 * rec * S, 2))
        alone['against_ns_median'] = round(alone['median_ms'] / base['median_ms'], 3)
        full = StreamMonitor(S, lag=1)
        row('StreamMonitor + stats, seg, nseg', S, timed(lambda i: full.process(speech[i % n], speech[(i - 1) % n], noise[i % n], want=WANT), a.hops, warmup))
        pair = (StreamMonitor(S, lag=1), StreamMonitor(S, lag=1))

        def both(i):
            pair[0].process(speech[i % n], speech[(i - 1) % n], noise[i % n])
            pair[1].process(speech[i % n], None, noise[i % n])
        row('StreamMonitor, processed and baseline', S, timed(both, a.hops, warmup))
        del mon, full, pair
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, 'w') as f:
            json.dump({'rows': rows}, f, indent=1)


if __name__ == '__main__':
    main()
