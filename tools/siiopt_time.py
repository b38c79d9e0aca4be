"""Device time of the SII-optimal rule (nele_gan_amd/siiopt.py) beside the generator it replaces:
python tools/siiopt_time.py [--hops N] [--warmup W] [--streams 1,16,256,1024,4096] [--json PATH]

(1) The real-time hop: for every B, RealtimeEnhancer(rule=SiiOptRule()) and RealtimeEnhancer() (the generator, bf16) on device inputs, W
    warm-up hops and N timed hops each between two HIP events, a 0.3 ms idle kernel queued before each timed hop - the method of
    tools/realtime_time.py.  Median and p99 per configuration.
(2) The offline mask at 128 x 8 s (T = 501): nele_siiopt_mask beside Generator_Conv1D_cLN's forward pass (bf16, weights frozen), 50 calls
    each after 5, median.
One JSON line per measurement."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nele_gan_amd import _lib, model, synth  # noqa: E402
from nele_gan_amd.realtime import HOP, RealtimeEnhancer  # noqa: E402
from nele_gan_amd.siiopt import SiiOptRule  # noqa: E402


def hop_time(rt, S, hops, warmup, audio):
    c, v = audio
    reps = (S + c.shape[0] - 1) // c.shape[0]
    c = np.tile(c, (reps, 1))[:S]
    v = np.tile(v, (reps, 1))[:S]
    nh_audio = c.shape[1] // HOP
    dc = [torch.from_numpy(np.ascontiguousarray(c[:, h * HOP:(h + 1) * HOP])).cuda() for h in range(nh_audio)]
    dn = [torch.from_numpy(np.ascontiguousarray(v[:, h * HOP:(h + 1) * HOP])).cuda() for h in range(nh_audio)]
    st = _lib.stream()
    ms, pend = [], []
    for i in range(warmup + hops):
        h = i % nh_audio
        if h == 0 and i > 0:
            rt.reset(range(S))
        _lib.lib.nele_stream_spin(300.0, st)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rt.process(dc[h], dn[h])
        e1.record()
        if i >= warmup:
            pend.append((e0, e1))
        if len(pend) >= 256 or i == warmup + hops - 1:      # a bounded number of live events
            torch.cuda.synchronize()
            ms.extend(x.elapsed_time(y) for x, y in pend)
            pend = []
    ms = np.array(ms)
    return float(np.median(ms)), float(np.percentile(ms, 99)), len(ms)


def call_time(fn, n=50, warmup=5):
    st = _lib.stream()
    ms = []
    for i in range(warmup + n):
        _lib.lib.nele_stream_spin(300.0, st)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hops', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--streams', default='1,16,256,1024,4096')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    audio = synth.batch(16, 256 * 300, start=900)
    rows = []
    for S in [int(s) for s in a.streams.split(',')]:
        row = {'streams': S, 'hops': a.hops}
        for tag, make in (('rule', lambda: RealtimeEnhancer(rule=SiiOptRule(), streams=S)), ('generator_bf16', lambda: RealtimeEnhancer(streams=S))):
            rt = make()
            med, p99, _ = hop_time(rt, S, a.hops, a.warmup, audio)
            del rt
            torch.cuda.empty_cache()
            row[tag + '_median_ms'], row[tag + '_p99_ms'] = round(med, 4), round(p99, 4)
        row['p99_generator_over_rule'] = round(row['generator_bf16_p99_ms'] / row['rule_p99_ms'], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    B, T = 128, 501
    g = torch.Generator().manual_seed(1)
    cb = torch.rand((B, T, 64), generator=g).cuda()
    nb = torch.rand((B, T, 64), generator=g).cuda()
    rule = SiiOptRule()
    G = model.Generator_Conv1D_cLN().cuda().eval()
    G.precision = 'bf16'
    G.freeze_weights('cuda')
    with torch.no_grad():
        off = {'B': B, 'T': T, 'siiopt_mask_ms': round(call_time(lambda: rule(cb, nb)), 4),
               'generator_bf16_forward_ms': round(call_time(lambda: G(cb, nb)), 4)}
    print(json.dumps(off), flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump({'hop': rows, 'offline': off}, f, indent=1)


if __name__ == '__main__':
    main()
