"""Per-hop device time of the bulk-delay search (nele_gan_amd/bulkdelay.py): python tools/bulk_time.py [--hops N] [--warmup W]
[--streams 1,16,256,1024,4096] [--blocks 8,32] [--partitions 8,32] [--json PATH]

For every streams value, in one run:
  EchoCanceller at each --partitions (the yardstick: a hop of comparable transforms and traffic);
  BulkDelay with every slot searching: hold is set beyond the run so that no slot locks, and every 4 * blocks hops all slots are reset,
    behind a timed hop's closing event and so outside every timed span.  The blocks - 1 hops behind a reset only fill the sums; the
    hops that also evaluate (the steady state of a search) are the figure reported, the filling hops are printed apart;
  BulkDelay with every slot locked (set_delay);
  the composite AlignedEchoCanceller(BulkDelay(blocks), EchoCanceller(4)) with every slot locked.
W warm-up hops, then N timed hops of one hop per call on device inputs, each between two HIP events on the current stream, a 0.3 ms
idle kernel (nele_stream_spin) queued ahead of each so that the host's enqueue never shows up as device time.  Prints one JSON line per
configuration (median and p99); traffic_bytes_per_stream_hop is the searching hop's count of bytes read and written per stream."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nele_gan_amd import _lib, synth  # noqa: E402
from nele_gan_amd.aec import HOP, EchoCanceller  # noqa: E402
from nele_gan_amd.bulkdelay import AlignedEchoCanceller, BulkDelay  # noqa: E402


def timed(step, hops, warmup, between=None):
    """between(i): queued behind hop i's closing event, outside every timed span"""
    st = _lib.stream()
    ms, pend = [], []
    for i in range(warmup + hops):
        _lib.lib.nele_stream_spin(300.0, st)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step(i)
        e1.record()
        if between is not None:
            between(i)
        if i >= warmup:
            pend.append((i, e0, e1))
        if len(pend) >= 256 or i == warmup + hops - 1:      # a bounded number of live events
            torch.cuda.synchronize()
            ms.extend((k, x.elapsed_time(y)) for k, x, y in pend)
            pend = []
    return ms


def stats(ms):
    v = np.array([m for _, m in ms])
    return {'median_ms': round(float(np.median(v)), 4), 'p99_ms': round(float(np.percentile(v, 99)), 4), 'hops': len(v)}


def device_hops(a, S):
    reps = (S + a.shape[0] - 1) // a.shape[0]
    a = np.tile(a, (reps, 1))[:S]
    return [torch.from_numpy(np.ascontiguousarray(a[:, h * HOP:(h + 1) * HOP])).cuda() for h in range(a.shape[1] // HOP)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hops', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--streams', default='1,16,256,1024,4096')
    ap.add_argument('--blocks', default='8,32')
    ap.add_argument('--partitions', default='8,32')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    far, near = synth.batch(16, HOP * 100, start=900)
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    for S in [int(s) for s in a.streams.split(',')]:
        played, noise = device_hops(far, S), device_hops(near, S)
        mic = [n + 0.5 * torch.roll(p, 40, dims=1) for n, p in zip(noise, played)]        # any signal: the work does not depend on the data
        n = len(played)
        aec_med = {}
        for P in [int(p) for p in a.partitions.split(',')]:
            aec = EchoCanceller(S, partitions=P)
            r = dict({'what': 'EchoCanceller', 'streams': S, 'partitions': P}, **stats(timed(lambda i: aec.process(mic[i % n], played[i % n]), a.hops, a.warmup)))
            aec_med[P] = r['median_ms']
            emit(r)
            del aec
            torch.cuda.empty_cache()
        for Q in [int(q) for q in a.blocks.split(',')]:
            every = list(range(S))
            # searching: hold beyond the run, so that no slot locks; the sums are cleared every 4 Q hops, outside the timed spans, and
            # the Q - 1 hops behind a reset, which do not evaluate, are reported apart
            bd = BulkDelay(S, blocks=Q, hold=1 << 30)
            ms = timed(lambda i: bd.process(mic[i % n], played[i % n]), a.hops, a.warmup, between=lambda i: bd.reset(every) if i % (4 * Q) == 4 * Q - 1 else None)
            ev = [(k, m) for k, m in ms if k % (4 * Q) >= Q - 1]
            fill = [(k, m) for k, m in ms if k % (4 * Q) < Q - 1]
            rec = int(_lib.lib.nele_bulk_stream_record_bytes(Q))
            traffic = 2 * 1024 + 3 * 1024 + 16 * 256 * (3 * Q + 1) + 4 * 8 * 264 + 8 * Q  # x, d read; line, out written, x_prev read (its write-back is per call); X ring read, X_0 written, C read and written; S_d, S_x read and written; e
            r = dict({'what': 'BulkDelay searching', 'streams': S, 'blocks': Q, 'record_bytes': rec, 'traffic_bytes_per_stream_hop': traffic}, **stats(ev))
            r['share_of_16ms_hop'] = round(r['p99_ms'] / 16.0, 4)
            r['GB_per_s_at_median'] = round(S * traffic / (r['median_ms'] * 1e-3) / 1e9, 1)
            r['against_EchoCanceller_median'] = {str(P): round(r['median_ms'] / v, 3) for P, v in aec_med.items()}
            emit(r)
            if fill:
                emit(dict({'what': 'BulkDelay searching, hops that only fill the sums', 'streams': S, 'blocks': Q}, **stats(fill)))
            bd.set_delay(every, Q - 1)
            r = dict({'what': 'BulkDelay locked', 'streams': S, 'blocks': Q}, **stats(timed(lambda i: bd.process(mic[i % n], played[i % n]), a.hops, a.warmup)))
            r['share_of_16ms_hop'] = round(r['p99_ms'] / 16.0, 4)
            emit(r)
            comp = AlignedEchoCanceller(bd, EchoCanceller(S, partitions=4))
            r = dict({'what': 'AlignedEchoCanceller locked, P = 4', 'streams': S, 'blocks': Q},
                     **stats(timed(lambda i: comp.process(mic[i % n], played[i % n]), a.hops, a.warmup)))
            r['share_of_16ms_hop'] = round(r['p99_ms'] / 16.0, 4)
            emit(r)
            del comp, bd
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, 'w') as f:
            json.dump({'rows': rows}, f, indent=1)


if __name__ == '__main__':
    main()
