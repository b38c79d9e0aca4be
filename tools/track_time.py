"""Per-hop device time of the delay tracker (nele_gan_amd/bulktrack.py): python tools/track_time.py [--hops N] [--warmup W]
[--streams 1,16,256,1024,4096] [--blocks 32] [--patience 128] [--rest 384] [--json PATH]

For every streams value, in one run:
  BulkDelay with every slot searching and with every slot locked, as tools/bulk_time.py measures them (the yardsticks);
  TrackingBulkDelay, every slot locked by set_delay, rest = 0: every hop is a searching hop, and every `patience`-th one ends with the
    give-up's clear of the ring and C_q (hold is set beyond the run, so that a search ends by its patience alone; what a search finds
    does not change its work); the hops with a clear are also listed apart;
  TrackingBulkDelay with --rest (384 behind a patience of 128: a search runs on a quarter of the hops): all hops, and the searching and
    the resting hops apart; the mean is the figure that shows the duty;
  the composite TrackedEchoCanceller(TrackingBulkDelay(blocks), EchoCanceller(4)) at rest = 0.
W warm-up hops, then N timed hops of one hop per call on device inputs, each between two HIP events on the current stream, a 0.3 ms
idle kernel (nele_stream_spin) queued ahead of each so that the host's enqueue never shows up as device time.  Prints one JSON line per
configuration (median, p99 and mean)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bulk_time import device_hops, timed  # noqa: E402  (tools/ is the script's directory)
from nele_gan_amd import _lib, synth  # noqa: E402
from nele_gan_amd.aec import HOP, EchoCanceller  # noqa: E402
from nele_gan_amd.bulkdelay import BulkDelay  # noqa: E402
from nele_gan_amd.bulktrack import TrackedEchoCanceller, TrackingBulkDelay  # noqa: E402


def stats(ms):
    v = np.array([m for _, m in ms])
    return {'median_ms': round(float(np.median(v)), 4), 'p99_ms': round(float(np.percentile(v, 99)), 4), 'mean_ms': round(float(v.mean()), 4),
            'hops': len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hops', type=int, default=1024)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--streams', default='1,16,256,1024,4096')
    ap.add_argument('--blocks', default='32')
    ap.add_argument('--patience', type=int, default=128)
    ap.add_argument('--rest', type=int, default=384)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    far, near = synth.batch(16, HOP * 100, start=900)
    rows = []

    def emit(r):
        r['share_of_16ms_hop'] = round(r['p99_ms'] / 16.0, 4)
        rows.append(r)
        print(json.dumps(r), flush=True)

    for S in [int(s) for s in a.streams.split(',')]:
        played, noise = device_hops(far, S), device_hops(near, S)
        mic = [n + 0.5 * torch.roll(p, 40, dims=1) for n, p in zip(noise, played)]        # any signal: the work does not depend on the data
        n = len(played)
        every = list(range(S))
        for Q in [int(q) for q in a.blocks.split(',')]:
            bd = BulkDelay(S, blocks=Q, hold=1 << 30)
            ms = timed(lambda i: bd.process(mic[i % n], played[i % n]), a.hops, a.warmup, between=lambda i: bd.reset(every) if i % (4 * Q) == 4 * Q - 1 else None)
            emit(dict({'what': 'BulkDelay searching', 'streams': S, 'blocks': Q}, **stats([(k, m) for k, m in ms if k % (4 * Q) >= Q - 1])))
            bd.set_delay(every, Q - 1)
            emit(dict({'what': 'BulkDelay locked', 'streams': S, 'blocks': Q}, **stats(timed(lambda i: bd.process(mic[i % n], played[i % n]), a.hops, a.warmup))))
            del bd
            torch.cuda.empty_cache()
            # hold beyond the run: a background search ends by its patience alone, on the hops i with (i + 1) % patience == 0
            tr = TrackingBulkDelay(S, blocks=Q, hold=1 << 30, patience=a.patience, rest=0)
            tr.set_delay(every, Q - 1)
            ms = timed(lambda i: tr.process(mic[i % n], played[i % n]), a.hops, a.warmup)
            emit(dict({'what': 'TrackingBulkDelay rest 0', 'streams': S, 'blocks': Q, 'patience': a.patience}, **stats(ms)))
            emit(dict({'what': 'TrackingBulkDelay rest 0, hops that clear', 'streams': S, 'blocks': Q}, **stats([(k, m) for k, m in ms if (k + 1) % a.patience == 0])))
            assert int(tr.status()['gaveups'][0].item()) == (a.warmup + a.hops) // a.patience and int(tr.moves().max().item()) == 0
            comp = TrackedEchoCanceller(tr, EchoCanceller(S, partitions=4))
            emit(dict({'what': 'TrackedEchoCanceller rest 0, P = 4', 'streams': S, 'blocks': Q},
                      **stats(timed(lambda i: comp.process(mic[i % n], played[i % n]), a.hops, a.warmup))))
            del comp, tr
            torch.cuda.empty_cache()
            cycle = a.patience + a.rest
            tr = TrackingBulkDelay(S, blocks=Q, hold=1 << 30, patience=a.patience, rest=a.rest)
            tr.set_delay(every, Q - 1)
            ms = timed(lambda i: tr.process(mic[i % n], played[i % n]), a.hops, a.warmup)
            duty = round(a.patience / cycle, 3)
            emit(dict({'what': 'TrackingBulkDelay rest %d' % a.rest, 'streams': S, 'blocks': Q, 'patience': a.patience, 'duty': duty}, **stats(ms)))
            emit(dict({'what': 'TrackingBulkDelay rest %d, searching hops' % a.rest, 'streams': S, 'blocks': Q},
                      **stats([(k, m) for k, m in ms if k % cycle < a.patience])))
            emit(dict({'what': 'TrackingBulkDelay rest %d, resting hops' % a.rest, 'streams': S, 'blocks': Q},
                      **stats([(k, m) for k, m in ms if k % cycle >= a.patience])))
            del tr
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, 'w') as f:
            json.dump({'rows': rows}, f, indent=1)


if __name__ == '__main__':
    main()
