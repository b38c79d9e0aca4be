"""Per-layer error of the convolution entry points in the three operand precisions against float64 torch, on random N(0, 1) operands at
T = 251: max |error| / sum |a*b| over the outputs of the forward pass, the data gradient (the same convolution with the channel counts
swapped, as the plans run it) and the weight gradient.  Prints one JSON line (the table of DESIGN 4.1).
    python tools/precision_error.py [T]"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nele_gan_amd import _lib as L  # noqa: E402
from nele_gan_amd import ops  # noqa: E402,F401

# (name, C, N, KH, KW, H): G's Conv1d layers and D.layers.1-4 (D at 16 output rows)
LAYERS = [('G.conv0', 128, 256, 1, 5, 1), ('G.conv1-4', 256, 256, 1, 7, 1), ('G.conv5', 256, 64, 1, 5, 1), ('D.layers.1', 8, 16, 3, 3, 16),
          ('D.layers.2', 16, 32, 5, 5, 16), ('D.layers.3', 32, 48, 7, 7, 16), ('D.layers.4', 48, 64, 9, 9, 16)]


def geom(B, H, W, C, KH, KW, N):
    Ho, Wo = H - KH + 1, W - KW + 1
    return (ctypes.c_int * 15)(H, W, C, 0, 0, Ho, Wo, KW * C, W * C, KH * KW * C, Ho, Wo, N, 0, 0), B * Ho * Wo, Ho, Wo


def conv(A, Wt, prec):
    B, H, W, C = A.shape
    N, _, KH, KW = Wt.shape
    g, M, Ho, Wo = geom(B, H, W, C, KH, KW, N)
    Wg = Wt.permute(0, 2, 3, 1).reshape(N, -1).contiguous()
    out = torch.zeros((B, Ho, Wo, N), device='cuda')
    s, ne = L.stream(), int(L.lib.nele_weight_frag16_elems(N, KW * C, KH))
    if prec == 'bf16x3' and L.lib.nele_conv_span_bf16x3_supported(M, N, g, KH, KW):
        hi, lo = torch.empty(ne, dtype=torch.bfloat16, device='cuda'), torch.empty(ne, dtype=torch.bfloat16, device='cuda')
        L.call('nele_weight_prep_frag16x3', L.ptr(Wg), N, Wg.shape[1], KW * C, KH, L.ptr(hi), L.ptr(lo), s)
        L.call('nele_conv_span_bf16x3', L.ptr(A), L.ptr(hi), L.ptr(lo), None, None, L.ptr(out), M, N, 0, 0.0, g, KH, KW, A.numel(), s)
        kind = 'split'
    elif prec == 'bf16' and L.lib.nele_conv_span_bf16_supported(M, N, g, KH, KW):
        wf = torch.empty(ne, dtype=torch.bfloat16, device='cuda')
        L.call('nele_weight_prep_frag16', L.ptr(Wg), N, Wg.shape[1], KW * C, KH, L.ptr(wf), s)
        L.call('nele_conv_span_bf16', L.ptr(A), L.ptr(wf), None, None, L.ptr(out), M, N, 0, 0.0, g, KH, KW, A.numel(), s)
        kind = 'bf16'
    else:
        L.call('nele_conv_gemm', L.ptr(A), L.ptr(Wg), None, None, L.ptr(out), M, N, 0, 0.0, g, s)
        kind = 'f32'
    torch.cuda.synchronize()
    return out, kind


def wgrad(A, dO, KH, KW, prec):
    B, H, W, C = A.shape
    N = dO.shape[-1]
    g, M, _, _ = geom(B, H, W, C, KH, KW, N)
    nws = int(L.lib.nele_conv_wgrad_workspace_floats(M, N, KH * KW * C, None))
    ws, dW, db = torch.empty(nws, device='cuda'), torch.zeros((N, C, KH, KW), device='cuda'), torch.empty(N, device='cuda')
    fn = {'f32': 'nele_conv_wgrad', 'bf16': 'nele_conv_wgrad_bf16', 'bf16x3': 'nele_conv_wgrad_bf16x3'}[prec]
    L.call(fn, L.ptr(A), L.ptr(dO), L.ptr(ws), nws, M, N, g, KH, KW, C, L.ptr(dW), L.ptr(db), 0, L.stream())
    torch.cuda.synchronize()
    return dW


def err(got, ref, scale):
    return float(((got.double() - ref).abs() / scale.clamp_min(1e-30)).max())


def main():
    T = int(sys.argv[1]) if len(sys.argv) > 1 else 251
    gen = torch.Generator(device='cuda').manual_seed(5)
    rows = []
    for name, C, N, KH, KW, H in LAYERS:
        B = 4 if KH == 1 else 1
        for pas, (c, n) in (('forward', (C, N)), ('data gradient', (N, C))):
            A = torch.randn((B, H + KH - 1 if KH > 1 else 1, T + KW - 1, c), device='cuda', generator=gen)
            Wt = torch.randn((n, c, KH, KW), device='cuda', generator=gen)
            An, Wd = A.permute(0, 3, 1, 2).double(), Wt.double()
            ref = torch.nn.functional.conv2d(An, Wd).permute(0, 2, 3, 1)
            sc = torch.nn.functional.conv2d(An.abs(), Wd.abs()).permute(0, 2, 3, 1)
            row = {'layer': name, 'pass': pas}
            for p in ('f32', 'bf16x3', 'bf16'):
                out, kind = conv(A, Wt, p)
                row[p] = float('%.2e' % err(out, ref, sc))
                row[p + '_kernel'] = kind
            rows.append(row)
            if pas == 'forward':
                dO = torch.randn(ref.shape, device='cuda', generator=gen)
                dOn = dO.permute(0, 3, 1, 2).double()
                rW = torch.nn.grad.conv2d_weight(An, Wt.shape, dOn)
                sW = torch.nn.grad.conv2d_weight(An.abs(), Wt.shape, dOn.abs())
                wrow = {'layer': name, 'pass': 'weight gradient'}
                for p in ('f32', 'bf16x3', 'bf16'):
                    wrow[p] = float('%.2e' % err(wgrad(A, dO.contiguous(), KH, KW, p), rW, sW))
                rows.append(wrow)
    print(json.dumps({'T': T, 'metric': 'max |error| / sum |a*b| against float64', 'rows': rows}))


if __name__ == '__main__':
    main()
