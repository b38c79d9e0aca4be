"""Per-hop device time of the clock-drift compensator (nele_gan_amd/drift.py): python tools/drift_time.py [--hops N] [--warmup W]
[--streams 1,16,256,1024,4096] [--blocks 32] [--json PATH]

For every streams value, in one run:
  DriftCompensator, every slot snapped to base blocks - 1 and started at +100 ppm (the warp, the estimator and the loop on every hop);
  TrackingBulkDelay, every slot locked by set_delay, rest 0 and rest 384 behind a patience of 128 (its locked hop: the yardstick that
    stands where the compensator's delay line stands);
  EchoCanceller with P = 4 (the stage behind it);
  the composite DriftTrackedEchoCanceller(TrackingBulkDelay(rest 384), DriftCompensator, EchoCanceller(4)).
W warm-up hops, then N timed hops of one hop per call on device inputs, each between two HIP events on the current stream, a 0.3 ms
idle kernel (nele_stream_spin) queued ahead of each so that the host's enqueue never shows up as device time.  Prints one JSON line per
configuration (median, p99 and mean)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bulk_time import device_hops, timed  # noqa: E402  (tools/ is the script's directory)
from track_time import stats  # noqa: E402
from nele_gan_amd import synth  # noqa: E402
from nele_gan_amd.aec import HOP, EchoCanceller  # noqa: E402
from nele_gan_amd.bulktrack import TrackingBulkDelay  # noqa: E402
from nele_gan_amd.drift import DriftCompensator, DriftTrackedEchoCanceller  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hops', type=int, default=1024)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--streams', default='1,16,256,1024,4096')
    ap.add_argument('--blocks', default='32')
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
            base = torch.full((S,), Q - 1, dtype=torch.int32, device='cuda')
            dc = DriftCompensator(S, blocks=Q)
            dc.set_rate(every, 100.0)
            emit(dict({'what': 'DriftCompensator', 'streams': S, 'blocks': Q},
                      **stats(timed(lambda i: dc.process(mic[i % n], played[i % n], base), a.hops, a.warmup))))
            assert int(dc.status()['n'].min().item()) == a.hops + a.warmup
            for rest in (0, 384):
                tr = TrackingBulkDelay(S, blocks=Q, hold=1 << 30, patience=128, rest=rest)
                tr.set_delay(every, Q - 1)
                emit(dict({'what': 'TrackingBulkDelay locked, rest %d' % rest, 'streams': S, 'blocks': Q},
                          **stats(timed(lambda i: tr.process(mic[i % n], played[i % n]), a.hops, a.warmup))))
            aec = EchoCanceller(S, partitions=4)
            emit(dict({'what': 'EchoCanceller P = 4', 'streams': S}, **stats(timed(lambda i: aec.process(mic[i % n], played[i % n]), a.hops, a.warmup))))
            comp = DriftTrackedEchoCanceller(tr, dc, aec)
            emit(dict({'what': 'DriftTrackedEchoCanceller rest 384, P = 4', 'streams': S, 'blocks': Q},
                      **stats(timed(lambda i: comp.process(mic[i % n], played[i % n]), a.hops, a.warmup))))
            del comp, tr, dc, aec
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, 'w') as f:
            json.dump({'rows': rows}, f, indent=1)


if __name__ == '__main__':
    main()
