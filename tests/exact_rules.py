"""The rules and helpers the kernel-level float64 tests share (test_bf16_exact_gpu.py, test_f32_exact_gpu.py, test_glue_exact_gpu.py).

Every reference runs in float64 on the SAME values the kernel reads.  The only legitimate difference is then the float32 accumulation
order, plus one bf16 rounding where a result is stored as bf16.  With S = sum |a * w| (the same operation on absolute values), per element:

  * float32 outputs:  |got - ref| <= 2e-5 S
  * bf16 outputs:     |got - ref| <= 2e-5 S + 2^-8 |ref|

The largest measured |got - ref| / S per kernel is collected in MARGINS and written as JSON to $NELE_EXACT_MARGINS when that variable is
set (the module-scoped fixture _report_margins, which every module that uses _check imports).
"""
import ctypes
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')
F = torch.nn.functional

from f32_cases import D_CONVS, G_LAYERS, d_dims as _d_dims  # noqa: E402,F401  (the networks' layer lists, kept free of torch for the CPU tests)

SLOPE = 0.3
EPI_NONE, EPI_BIAS, EPI_BIAS_LRELU, EPI_MASK_LRELU_GRAD, EPI_BIAS_EXPTANH = 0, 1, 2, 3, 4
ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -5         # csrc/common.h
C32 = 2e-5                       # float32 accumulation, relative to S
R16 = 2.0 ** -8                  # one bf16 rounding of the stored value
MARGINS = {}
P_ = ctypes.c_void_p


def _lib():
    from nele_gan_amd import _lib as L
    from nele_gan_amd import ops  # noqa: F401  (declares the dense / conv16 / cLN / head entry points)
    return L


@pytest.fixture(scope='module', autouse=True)
def _report_margins():
    yield
    path = os.environ.get('NELE_EXACT_MARGINS')
    if path:
        old = {}
        if os.path.exists(path):
            with open(path) as f:
                old = json.load(f)
        for k, v in MARGINS.items():
            old[k] = max(v, old.get(k, 0.0))
        with open(path, 'w') as f:
            json.dump(old, f, indent=1, sort_keys=True)


def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


def _r16(x):
    """float32 values that are exactly representable in bf16 (RNE)"""
    return x.to(torch.bfloat16).float()


def _lrelu(x):
    return torch.where(x > 0, x, SLOPE * x)


def _geom(H, W, C, Hout, Wout, KH, KW, OH, OW, OC, ih0=0, iw0=0, oh0=0, ow0=0):
    """ConvGeom of include/nele_hip.h (netplan.hip mk_geom)"""
    return (ctypes.c_int * 15)(H, W, C, ih0, iw0, Hout, Wout, KW * C, W * C, KH * KW * C, OH, OW, OC, oh0, ow0)


def _check(name, got, ref, S, bf16_out=False, c=C32, what=''):
    """the rule above; records the largest |got - ref| / S (less the bf16 rounding allowance) of the kernel `name`"""
    err = (got.double() - ref).abs()
    if bf16_out:
        err = err - R16 * ref.abs()
    ok = err <= c * S                                         # NaN (an element never written) fails
    ratio = (err.clamp_min(0) / S.clamp_min(1e-300))
    worst = float(ratio[torch.isfinite(ratio)].max()) if bool(torch.isfinite(ratio).any()) else float('nan')
    MARGINS[name] = max(MARGINS.get(name, 0.0), worst)
    if not bool(ok.all()):
        bad = ~ok
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError('%s %s: %d of %d elements beyond %.0e S (worst %.3g S); first at %s: got %r ref %r S %r' % (
            name, what, int(bad.sum()), bad.numel(), c, worst, idx, float(got[idx]), float(ref[idx]), float(S[idx])))


def _conv(A, Wt):
    """A [B][H][W][C] (NHWC), Wt [N][C][KH][KW] -> valid convolution [B][Hout][Wout][N] and S, both float64"""
    A, Wt = A.double(), Wt.double()
    r = F.conv2d(A.permute(0, 3, 1, 2), Wt).permute(0, 2, 3, 1)
    s = F.conv2d(A.abs().permute(0, 3, 1, 2), Wt.abs()).permute(0, 2, 3, 1)
    return r, s


def _wgrad_ref(A, dO, shape):
    """A [B][H][W][C], dO [B][Hout][Wout][N] -> dW [N][C][KH][KW] of the valid convolution and S, float64"""
    A, dO = A.double().permute(0, 3, 1, 2), dO.double().permute(0, 3, 1, 2)
    return torch.nn.grad.conv2d_weight(A, shape, dO), torch.nn.grad.conv2d_weight(A.abs(), shape, dO.abs())


def _fwd_layout(Wt):
    """[N][C][KH][KW] -> forward GEMM layout [N][KH * KW * C] (nele_weight_prep's Wf)"""
    return Wt.permute(0, 2, 3, 1).reshape(Wt.shape[0], -1).contiguous()


def _flip_layout(Wt):
    """[N][C][KH][KW] -> data-gradient GEMM layout Wb[c][KH-1-kh][KW-1-kw][n] as [C][KH * KW * N]"""
    return Wt.flip(2, 3).permute(1, 2, 3, 0).reshape(Wt.shape[1], -1).contiguous()


def _flip_weight(Wt):
    """the data gradient of a valid convolution = a valid convolution of the zero-bordered gradient with these weights"""
    return Wt.flip(2, 3).transpose(0, 1)


def _bordered(B, H, W, C, p, interior, dtype):
    """zero-bordered buffer [B][H + 2p][W + 2p][C] with `interior` (a tensor or a fill value) inside"""
    buf = torch.zeros((B, H + 2 * p, W + 2 * p, C), dtype=dtype, device='cuda')
    buf[:, p:p + H, p:p + W] = interior
    return buf


def _border_is_zero(buf, p, what):
    if p == 0:
        return
    inner = torch.zeros(buf.shape[:3], dtype=torch.bool, device=buf.device)
    inner[:, p:-p, p:-p] = True
    border = buf[~inner]
    assert bool((border == 0).all()), '%s: the zero border was written (%d elements)' % (what, int((border != 0).sum()))


def _mlp(nout, seed):
    """random head (fc1 64->64, fc2 64->16, fc3 16->nout, spectral-norm sigmas) -> tensors and the host pointer array of nele_gap_mlp_*"""
    g = _gen(seed)
    ws = [torch.randn(shape, device='cuda', generator=g) / np.sqrt(shape[1]) for shape in ((64, 64), (16, 64), (nout, 16))]
    bs = [0.1 * torch.randn(n, device='cuda', generator=g) for n in (64, 16, nout)]
    sg = [torch.tensor([s], device='cuda') for s in (1.3, 0.9, 1.7)]
    host = (P_ * 9)(*[t.data_ptr() for q in range(3) for t in (ws[q], bs[q], sg[q])])
    return ws, bs, sg, host


def _head_ref(pooled, ws, bs, sg):
    """float64 head on pooled [B][64]: values and propagated magnitudes (S of every stage)"""
    x, s = pooled.double(), pooled.double().abs()
    outs = []
    for q in range(3):
        w = ws[q].double() / sg[q].double()
        z, s = x @ w.T + bs[q].double(), s @ w.abs().T + bs[q].double().abs()
        x = _lrelu(z) if q < 2 else torch.sigmoid(z)
        outs.append((x, s))
    return outs
