"""Per-hop device time of the real-time enhancer (nele_gan_amd/realtime.py): python tools/realtime_time.py [--hops N] [--warmup W]
[--streams 1,16,256,1024,4096] [--prec f32,bf16] [--json PATH]

For every (streams, precision): W warm-up hops, then N timed hops, each between two HIP events on the enhancer's stream, once on device
inputs ('device') and once with the pinned host -> device copies of the hop's clean / noise and the device -> host copy of its output
('copies').  A 0.3 ms idle kernel (nele_stream_spin) is queued before each timed hop so that the host's enqueue never shows up as device
time.  Prints median and p99 per configuration and the real-time capacity: the largest B whose p99 hop time stays under 16 ms (one hop).
--trace: 20 hops of B = 16 only, for one `rocprofv3 --kernel-trace --stats` run (launches per hop)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nele_gan_amd import _lib, synth  # noqa: E402
from nele_gan_amd.realtime import HOP, RealtimeEnhancer  # noqa: E402


def run(S, prec, hops, warmup, copies, audio):
    rt = RealtimeEnhancer(streams=S, precision=prec)
    c, v = audio
    reps = (S + c.shape[0] - 1) // c.shape[0]
    c = np.tile(c, (reps, 1))[:S]
    v = np.tile(v, (reps, 1))[:S]
    nh_audio = c.shape[1] // HOP
    hc = [torch.from_numpy(np.ascontiguousarray(c[:, h * HOP:(h + 1) * HOP])).pin_memory() for h in range(nh_audio)]
    hn = [torch.from_numpy(np.ascontiguousarray(v[:, h * HOP:(h + 1) * HOP])).pin_memory() for h in range(nh_audio)]
    dc = [t.cuda() for t in hc]
    dn = [t.cuda() for t in hn]
    host_out = torch.empty((S, HOP), dtype=torch.float32).pin_memory()
    st = _lib.stream()
    ms, pend = [], []
    for i in range(warmup + hops):
        h = i % nh_audio
        if h == 0 and i > 0:
            rt.reset(range(S))
        _lib.lib.nele_stream_spin(300.0, st)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if copies:
            out = rt.process(hc[h], hn[h])
            host_out.copy_(out, non_blocking=True)
        else:
            out = rt.process(dc[h], dn[h])
        e1.record()
        if i >= warmup:
            pend.append((e0, e1))
        if len(pend) >= 256 or i == warmup + hops - 1:      # a bounded number of live events
            torch.cuda.synchronize()
            ms.extend(x.elapsed_time(y) for x, y in pend)
            pend = []
    ms = np.array(ms)
    del rt
    torch.cuda.empty_cache()
    return float(np.median(ms)), float(np.percentile(ms, 99)), len(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hops', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--streams', default='1,16,256,1024,4096')
    ap.add_argument('--prec', default='f32,bf16')
    ap.add_argument('--json', default=None)
    ap.add_argument('--trace', action='store_true')
    a = ap.parse_args()
    audio = synth.batch(16, 256 * 300, start=900)
    if a.trace:
        rt = RealtimeEnhancer(streams=16, precision='bf16')
        x = torch.from_numpy(np.ascontiguousarray(audio[0][:, :HOP * 20])).cuda()
        y = torch.from_numpy(np.ascontiguousarray(audio[1][:, :HOP * 20])).cuda()
        torch.cuda.synchronize()
        for h in range(20):
            rt.process(x[:, h * HOP:(h + 1) * HOP].contiguous(), y[:, h * HOP:(h + 1) * HOP].contiguous())
        torch.cuda.synchronize()
        print('trace: 20 hops of B = 16, bf16')
        return
    rows = []
    for prec in a.prec.split(','):
        for S in [int(s) for s in a.streams.split(',')]:
            for copies in (False, True):
                med, p99, n = run(S, prec, a.hops, a.warmup, copies, audio)
                r = {'streams': S, 'precision': prec, 'mode': 'copies' if copies else 'device', 'median_ms': round(med, 4),
                     'p99_ms': round(p99, 4), 'hops': n}
                rows.append(r)
                print(json.dumps(r), flush=True)
    cap = {}
    for prec in a.prec.split(','):
        for mode in ('device', 'copies'):
            ok = [r['streams'] for r in rows if r['precision'] == prec and r['mode'] == mode and r['p99_ms'] < 16.0]
            cap['%s/%s' % (prec, mode)] = max(ok) if ok else 0
    print(json.dumps({'realtime_capacity_p99_under_16ms': cap}), flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump({'rows': rows, 'capacity': cap}, f, indent=1)


if __name__ == '__main__':
    main()
