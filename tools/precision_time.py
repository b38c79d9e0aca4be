"""Times the network paths in the three operand precisions ('f32', 'bf16x3', 'bf16') and prints one JSON line (milliseconds, medians over
--reps repetitions of HIP events, after --warmup untimed ones):
  g_fwd_bwd / d_fwd_bwd   G / D forward + backward at B = 256, T = 251
  g_eval                  G evaluation forward at 128 x 8 s (T = 501)
  step                    GanTrainer.canonical_step at BASELINE configs[2] (B = 256, L = 64 000, SIIB + HASPI + ESTOI)
  enhance / enhance_stream4   Enhancer.enhance and Enhancer.enhance_stream(inflight=4) per 128 x 8 s batch
    python tools/precision_time.py [--reps 10] [--warmup 3] [--only g_fwd_bwd,step] [--precisions f32,bf16x3,bf16]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def timed(fn, reps, warmup, join=False):
    """median milliseconds of fn() between two HIP events on the current stream (join: wait for every stream before the end event)"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        if join:
            torch.cuda.synchronize()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only', default='g_fwd_bwd,d_fwd_bwd,g_eval,step,enhance,enhance_stream4')
    ap.add_argument('--precisions', default='f32,bf16x3,bf16')
    a = ap.parse_args()
    from nele_gan_amd import model as mods
    from nele_gan_amd import synth
    from nele_gan_amd.inference import Enhancer
    from nele_gan_amd.train_nele import GanTrainer
    items = a.only.split(',')
    precs = a.precisions.split(',')
    res = {p: {} for p in precs}
    dev = 'cuda'
    g = torch.Generator(device=dev).manual_seed(1)
    if 'g_fwd_bwd' in items or 'g_eval' in items:
        G = mods.Generator_Conv1D_cLN().to(dev)
        B, T = 256, 251
        x, y = torch.rand((B, T, 64), device=dev, generator=g) + 0.1, torch.rand((B, T, 64), device=dev, generator=g) + 0.1
        gw = torch.randn((B, T, 64), device=dev, generator=g)
        xe, ye = torch.rand((128, 501, 64), device=dev, generator=g) + 0.1, torch.rand((128, 501, 64), device=dev, generator=g) + 0.1
        for p in precs:
            G.precision = p
            if 'g_fwd_bwd' in items:
                G.train()
                res[p]['g_fwd_bwd'] = timed(lambda: (G(x, y) * gw).sum().backward(), a.reps, a.warmup)
            if 'g_eval' in items:
                G.eval()
                with torch.no_grad():
                    res[p]['g_eval'] = timed(lambda: G(xe, ye), a.reps, a.warmup)
        del G
    if 'd_fwd_bwd' in items:
        D = mods.Discriminator(nout=3).to(dev)
        D.train()
        B, T = 256, 251
        din = torch.zeros((B, 64, T, 4), device=dev)
        din[..., :3] = torch.rand((B, 64, T, 3), device=dev, generator=g)
        din.requires_grad_(True)
        tgt = torch.rand((B, 3), device=dev, generator=g)
        for p in precs:
            D.precision = p
            res[p]['d_fwd_bwd'] = timed(lambda: torch.nn.functional.mse_loss(D.forward_packed(din), tgt).backward(), a.reps, a.warmup)
        del D
    if 'step' in items:
        c, v = synth.batch(256, 64000, start=20000)
        cw, nw = torch.from_numpy(c).to(dev), torch.from_numpy(v).to(dev)
        for p in precs:
            tr = GanTrainer('siib&haspi&estoi')
            tr.G.precision = tr.D.precision = p
            res[p]['step'] = timed(lambda: tr.canonical_step(cw, nw), a.reps, a.warmup, join=True)
            tr.check_status()
            del tr
    if 'enhance' in items or 'enhance_stream4' in items:
        c, v = synth.batch(64, 128000, start=5000)
        cw, nw = torch.from_numpy(c).to(dev).repeat(2, 1), torch.from_numpy(v).to(dev).repeat(2, 1)
        e = Enhancer()
        for p in precs:
            e.G.precision = p
            if 'enhance' in items:
                res[p]['enhance'] = timed(lambda: e.enhance(cw, nw), a.reps, a.warmup)
            if 'enhance_stream4' in items:
                n = 8
                res[p]['enhance_stream4'] = timed(lambda: [o for o in e.enhance_stream([(cw, nw)] * n, inflight=4)], max(2, a.reps // 4), 1,
                                                  join=True) / n
    out = {'unit': 'ms (median of HIP-event intervals)', 'shapes': {'g_fwd_bwd': 'B=256 T=251', 'd_fwd_bwd': 'B=256 T=251', 'g_eval': 'B=128 T=501',
                                                                    'step': 'B=256 L=64000 siib&haspi&estoi', 'enhance': 'B=128 L=128000 per batch',
                                                                    'enhance_stream4': 'B=128 L=128000 per batch, 4 in flight'},
           'ms': {p: {k: round(t, 3) for k, t in r.items()} for p, r in res.items()}, 'device': torch.cuda.get_device_name()}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
