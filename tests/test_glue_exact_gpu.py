"""GPU: the glue kernels of the networks (disc.hip, gen.hip) on their own, against float64 on the float32 values they read.

Spectral norm and its weight gradient, the discriminator's head from a float32 activation (forward, backward into a float32 gradient
buffer, weight gradient), Adam, the utterance-level energy normalisation (forward and backward), the exp(3.2 tanh) gradient, the column
sums and the layout kernels.  Dot products follow the S rule of tests/exact_rules.py (|got - ref| <= 2e-5 S, S = the same sum on absolute
values), sums of small integers and pure data movement are bit for bit, element-wise float32 arithmetic is bounded in ulps of its terms,
each bound derived where it is used.  ULP = 2^-23: an upper bound of one float32 ulp of x, relative to |x|.  The float64 restatements are
tests/glue_refs.py, which test_glue_refs_cpu.py holds to float64 autograd of oracle/nets.py.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import f32_cases as cases  # noqa: E402
import glue_refs as ref  # noqa: E402
from exact_rules import (C32, ERR_INVALID_ARG, MARGINS, P_, SLOPE, _border_is_zero, _bordered, _check, _gen, _head_ref, _lib, _lrelu, _mlp,  # noqa: E402,F401
                         _report_margins)

NAN = float('nan')
ULP = 2.0 ** -23
SLOPE32 = float(np.float32(SLOPE))          # the slope as the kernels see it


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device='cuda')


def _ints(shape, hi, g):
    return torch.randint(-hi, hi + 1, shape, device='cuda', generator=g).float()


def _bounded(name, got, want, bound, what=''):
    """|got - want| <= bound per element (NaN fails); records the largest |got - want| / bound as the margin of `name`"""
    err = (got.double() - want).abs()
    ok = err <= bound
    ratio = err / bound.clamp_min(1e-300)
    fin = torch.isfinite(ratio)
    MARGINS[name] = max(MARGINS.get(name, 0.0), float(ratio[fin].max()) if bool(fin.any()) else float('nan'))
    assert bool(ok.all()), '%s %s: %d of %d elements beyond the bound (worst %.3g of it)' % (name, what, int((~ok).sum()), ok.numel(), MARGINS[name])


# ------------------------------------------------------------------------------------------ spectral norm
# eight layers in one launch: K < 64, K no multiple of 64 (the wave-strided u loop) or of 1024 (the block-strided v loop), N = 3 .. 64
SN_SHAPES = [(3, 4), (8, 16), (16, 63), (64, 64), (3, 1025), (64, 3888), (8, 1025), (16, 3888)]


def _sn_layers(seed, zero=False):
    g = _gen(seed)
    Ws = [torch.zeros((N, K), device='cuda') if zero else torch.randn((N, K), device='cuda', generator=g) / np.sqrt(K) for N, K in SN_SHAPES]
    us = [torch.nn.functional.normalize(torch.randn(N, device='cuda', generator=g), dim=0) for N, K in SN_SHAPES]
    vs = [torch.nn.functional.normalize(torch.randn(K, device='cuda', generator=g), dim=0) for N, K in SN_SHAPES]
    return Ws, us, vs


def _sn_call(L, Ws, us, vs, n_iter, layers=None, dims=None):
    layers = len(Ws) if layers is None else layers
    ptrs = (P_ * (3 * max(layers, len(Ws))))(*[t.data_ptr() for W, u, v in zip(Ws, us, vs) for t in (W, u, v)])
    dims = dims or [d for W in Ws for d in W.shape]
    sigma = _nan(max(layers, len(Ws)))
    st = L.lib.nele_spectral_norm(ptrs, (ctypes.c_int * len(dims))(*dims), layers, L.ptr(sigma), n_iter, L.stream())
    torch.cuda.synchronize()
    return st, sigma


def test_spectral_norm_stage_by_stage():
    """One power iteration, each stage against float64 on the kernel's own previous stage: v against normalize(W^T u_in), u against
    normalize(W v_got), sigma against u_got . (W v_got).

    Bound of a normalised vector x / ||x||: the float32 dot products that make x follow the S rule, 2e-5 S_k (S = |W|^T |u|, or |W| |v|);
    the norm is accumulated in float64 from those float32 values and rounded to float32 once; 1 / norm and the product with it are one
    rounding each.  So |got_k - x_k / ||x||| <= 2e-5 S_k / ||x|| + 4 ULP |x_k| / ||x||: half an ulp each for the float32 norm, its reciprocal
    and the product, and the rest for the norm's own change under the perturbation of x (relative sqrt(sum dx^2) / ||x||, which for the
    <= 67 sequential float32 additions behind each x_k - 2^-24 each, independent in sign - stays below 2e-7).  sigma: the float64 dot
    product of float32 u and float32 W v: sum_n |u_n| 2e-5 S_n, plus one rounding."""
    L = _lib()
    Ws, us, vs = _sn_layers(11)
    u_in = [u.clone() for u in us]
    st, sigma = _sn_call(L, Ws, us, vs, 1)
    assert st == 0
    for l, (W, u0, u, v) in enumerate(zip(Ws, u_in, us, vs)):
        W64, what = W.double(), 'layer %d %s' % (l, tuple(W.shape))
        a, Sa = W64.t() @ u0.double(), W64.abs().t() @ u0.double().abs()
        na = a.norm()
        _bounded('nele_spectral_norm.v', v, a / na, C32 * Sa / na + 4 * ULP * a.abs() / na, what)
        wv, Sw = W64 @ v.double(), W64.abs() @ v.double().abs()
        nw = wv.norm()
        _bounded('nele_spectral_norm.u', u, wv / nw, C32 * Sw / nw + 4 * ULP * wv.abs() / nw, what)
        s = u.double() @ wv
        _bounded('nele_spectral_norm.sigma', sigma[l], s, C32 * (u.double().abs() @ Sw) + ULP * s.abs(), what)
        assert abs(float(v.double().norm()) - 1) < 1e-6 and abs(float(u.double().norm()) - 1) < 1e-6


def test_spectral_norm_without_an_iteration_leaves_u_and_v():
    """n_iter = 0 (eval mode): u and v bit-unchanged, sigma = u . (W v) by the S rule"""
    L = _lib()
    Ws, us, vs = _sn_layers(12)
    u_in, v_in = [u.clone() for u in us], [v.clone() for v in vs]
    st, sigma = _sn_call(L, Ws, us, vs, 0)
    assert st == 0
    for l, (W, u, v) in enumerate(zip(Ws, us, vs)):
        assert torch.equal(u, u_in[l]) and torch.equal(v, v_in[l]), l
        Sw = W.double().abs() @ v.double().abs()
        s = u.double() @ (W.double() @ v.double())
        _bounded('nele_spectral_norm.sigma', sigma[l], s, C32 * (u.double().abs() @ Sw) + ULP * s.abs(), 'n_iter=0 layer %d' % l)


def test_spectral_norm_of_a_zero_weight_is_finite():
    """W = 0: the 1e-12 floor of normalize keeps u, v and sigma finite (all zero)"""
    L = _lib()
    Ws, us, vs = _sn_layers(13, zero=True)
    st, sigma = _sn_call(L, Ws, us, vs, 1)
    assert st == 0
    for u, v in zip(us, vs):
        assert bool(torch.isfinite(u).all() and torch.isfinite(v).all())
    assert bool(torch.isfinite(sigma).all()) and float(sigma.abs().max()) == 0.0


def test_spectral_norm_rejects_nine_layers_and_65_rows():
    L = _lib()
    Ws, us, vs = _sn_layers(14)
    u_in = [u.clone() for u in us]
    W9, u9, v9 = Ws + [Ws[0]], us + [us[0].clone()], vs + [vs[0].clone()]
    st, sigma = _sn_call(L, W9, u9, v9, 1, layers=9)
    assert st == ERR_INVALID_ARG and bool(torch.isnan(sigma).all())
    W65 = torch.randn((65, 16), device='cuda')
    st, sigma = _sn_call(L, [W65], [torch.ones(65, device='cuda')], [torch.ones(16, device='cuda')], 1)
    assert st == ERR_INVALID_ARG and bool(torch.isnan(sigma).all())
    assert all(torch.equal(a, b) for a, b in zip(us, u_in))


# ------------------------------------------------------------------------------------------ nele_sn_grad
@pytest.mark.parametrize('N,K', [(3, 16), (64, 64), (17, 241), (64, 3888)])
def test_sn_grad_against_float64(N, K):
    """dst (+)= (dW - <dW, W / sigma> u v^T) / sigma with N K = 48, 4096 (one exact chunk), 4097 (chunk + 1) and 64 * 3888, accumulate 0
    and 1.  The dot product is accumulated in float64 from float32 products dW * (W * (1 / sigma)) (two roundings each): within 1e-6 of its
    magnitude sum.  The element is float32 arithmetic - float32(dot), * u, * v, the difference, * (1 / sigma): half an ulp each, on terms no
    larger than |dW| + |dot u v| - so 4 ULP (|dW| + |dot u v|) / sigma covers it; accumulate adds one rounding of old + value."""
    L = _lib()
    g = _gen(N * K)
    dW, W = torch.randn((N, K), device='cuda', generator=g), torch.randn((N, K), device='cuda', generator=g) / np.sqrt(K)
    u = torch.nn.functional.normalize(torch.randn(N, device='cuda', generator=g), dim=0)
    v = torch.nn.functional.normalize(torch.randn(K, device='cuda', generator=g), dim=0)
    sigma = torch.tensor([1.3], device='cuda')
    want, dot, Sdot = ref.sn_grad(dW.double(), W.double(), u.double(), v.double(), sigma.double())
    uv = torch.outer(u.double(), v.double()).abs()
    bound = (4 * ULP * (dW.double().abs() + dot.abs() * uv) + 1e-6 * Sdot * uv) / sigma.double()
    scratch = _nan(int(L.lib.nele_sn_grad_scratch_doubles(N * K)) + 2, dtype=torch.float64)
    assert scratch.numel() - 2 == -(-N * K // 4096)
    for acc in (0, 1):
        old = torch.randn((N, K), device='cuda', generator=g) if acc else None
        dst = _nan(N * K + 8)
        if acc:
            dst[:N * K] = old.flatten()
        L.call('nele_sn_grad', L.ptr(dW), L.ptr(W), L.ptr(u), L.ptr(v), L.ptr(sigma), N, K, L.ptr(dst), acc, L.ptr(scratch), L.stream())
        torch.cuda.synchronize()
        w = want + (old.double() if acc else 0)
        _bounded('nele_sn_grad', dst[:N * K].view(N, K), w, bound + (ULP * (old.double().abs() + want.abs()) if acc else 0), 'N=%d K=%d accumulate=%d' % (N, K, acc))
        assert bool(torch.isnan(dst[N * K:]).all()) and bool(torch.isnan(scratch[-2:]).all())
    # the rank-one term is there: without it the result would be off by |dot u v| / sigma, far beyond the bound
    assert float((dot.abs() * uv / sigma.double()).max()) > 100 * float(bound.max())


# ------------------------------------------------------------------------------------------ the head
def _layer_ref(x, w, b, sg, last):
    """one Linear(W / sigma) + activation in float64 on the float32 input x, and its magnitude sum"""
    wn = w.double() / sg.double()
    z, s = x.double() @ wn.T + b.double(), x.double().abs() @ wn.abs().T + b.double().abs()
    return (torch.sigmoid(z) if last else _lrelu(z)), s


@pytest.mark.parametrize('nout', [2, 3])
@pytest.mark.parametrize('B,Hout,Wout', [(1, 44, 32), (3, 44, 65)])
def test_head_forward_from_a_float32_activation(B, Hout, Wout, nout):
    """nele_gap_mlp_fwd (every column) and nele_gap_mlp_fwd_var (wvalid = 65, 41, 1) from act [B][Hout Wout][64] float32: pooled is the
    float64 mean rounded once to float32 (half an ulp: 2^-24 relative); h1, h2 and the score follow the S rule, each layer on the kernel's
    own previous output (dot products of 64 and 16 float32 products)."""
    L = _lib()
    P = Hout * Wout
    act = 0.05 + torch.randn((B, Hout, Wout, 64), device='cuda', generator=_gen(B + Wout + nout))
    ws, bs, sg, host = _mlp(nout, 40 + nout)
    for wv in (None, [65, 41, 1][:B] if B > 1 else [Wout - 3]):
        wvt = None if wv is None else torch.tensor(wv, dtype=torch.int32, device='cuda')
        pooled, h1, h2, score = _nan(B, 64), _nan(B, 64), _nan(B, 16), _nan(B, nout)
        scratch = _nan(B, 32, 64, dtype=torch.float64)
        if wv is None:
            L.call('nele_gap_mlp_fwd', L.ptr(act), B, P, host, nout, SLOPE, L.ptr(pooled), L.ptr(h1), L.ptr(h2), L.ptr(score), L.ptr(scratch), L.stream())
        else:
            L.call('nele_gap_mlp_fwd_var', L.ptr(act), B, P, Wout, L.ptr(wvt), host, nout, SLOPE, L.ptr(pooled), L.ptr(h1), L.ptr(h2), L.ptr(score),
                   L.ptr(scratch), L.stream())
        torch.cuda.synchronize()
        cols = [Wout] * B if wv is None else wv
        pref = torch.stack([act[b, :, :cols[b]].double().mean((0, 1)) for b in range(B)])
        what = 'B=%d Wout=%d nout=%d wvalid=%s' % (B, Wout, nout, wv)
        _bounded('nele_gap_mlp_fwd.pooled', pooled, pref, 2.0 ** -24 * pref.abs() * (1 + 1e-9), what)
        x = pooled
        for q, (name, got) in enumerate((('h1', h1), ('h2', h2), ('score', score))):
            r, s = _layer_ref(x, ws[q], bs[q], sg[q], q == 2)
            _check('nele_gap_mlp_fwd.' + name, got, r, s, what=what)
            x = got


@pytest.mark.parametrize('B,Hout,Wout,var', [(1, 44, 32, False), (3, 44, 65, True), (3, 5, 65, False)])
def test_head_backward_into_a_float32_gradient_buffer(B, Hout, Wout, var):
    """nele_gap_mlp_bwd and nele_gap_mlp_bwd_var (wvalid = 65, 41, 1) with a float32 gbuf against float64 autograd of the head: dz3, dz2, dz1
    and dpooled within 2e-5 of their propagated magnitudes; the pooling gradient dpooled / (Hout wvalid) LeakyReLU'(act) by the same rule
    inside the bordered buffer, exactly zero at columns >= wvalid[b], and the border still zero."""
    L = _lib()
    g = _gen(17 * Wout + B + Hout)
    p, nout = 8, 3
    ws, bs, sg, host = _mlp(nout, 5 * Wout + B)
    pooled = (0.2 * torch.randn((B, 64), device='cuda', generator=g)).double().requires_grad_(True)
    zs, x = [], pooled
    for q in range(3):
        z = x @ (ws[q].double() / sg[q].double()).T + bs[q].double()
        z.retain_grad()
        zs.append(z)
        x = _lrelu(z) if q < 2 else torch.sigmoid(z)
    h1, h2, score = _lrelu(zs[0]).float().detach(), _lrelu(zs[1]).float().detach(), x.float().detach()
    dscore = torch.randn((B, nout), device='cuda', generator=g)
    (x * dscore.double()).sum().backward()
    act = torch.randn((B, Hout, Wout, 64), device='cuda', generator=g)
    wv = [65, 41, 1][:B] if var else [Wout] * B
    wvt = torch.tensor(wv, dtype=torch.int32, device='cuda')
    dz3, dz2, dz1, dp = _nan(B, nout), _nan(B, 16), _nan(B, 64), _nan(B, 64)
    gb = _bordered(B, Hout, Wout, 64, p, NAN, torch.float32)
    if var:
        L.call('nele_gap_mlp_bwd_var', L.ptr(dscore), L.ptr(score), L.ptr(h1), L.ptr(h2), L.ptr(act), host, nout, SLOPE, B, Hout, Wout, L.ptr(wvt),
               Hout + 2 * p, Wout + 2 * p, p, p, L.ptr(dz3), L.ptr(dz2), L.ptr(dz1), L.ptr(dp), L.ptr(gb), L.stream())
    else:
        L.call('nele_gap_mlp_bwd', L.ptr(dscore), L.ptr(score), L.ptr(h1), L.ptr(h2), L.ptr(act), host, nout, SLOPE, B, Hout, Wout,
               Hout + 2 * p, Wout + 2 * p, p, p, L.ptr(dz3), L.ptr(dz2), L.ptr(dz1), L.ptr(dp), L.ptr(gb), L.stream())
    torch.cuda.synchronize()
    fn = 'nele_gap_mlp_bwd' + ('_var' if var else '')
    s = (dscore.double() * score.double() * (1 - score.double())).abs()
    for q, (name, got) in enumerate((('dz3', dz3), ('dz2', dz2), ('dz1', dz1))):
        _check(fn + '.' + name, got, zs[2 - q].grad, s)
        w = (ws[2 - q].double() / sg[2 - q].double()).abs()
        s = (s @ w) * (1.0 if q == 2 else torch.where(zs[1 - q].detach() > 0, 1.0, SLOPE))
    _check(fn + '.dpooled', dp, pooled.grad, s)
    want = ref.gap_backward(pooled.grad, act.double(), wv, SLOPE32)
    mag = ref.gap_backward(s, act.double().abs() + 1, wv, SLOPE32) * torch.where(act.double() > 0, 1.0, SLOPE32)
    inner = gb[:, p:p + Hout, p:p + Wout]
    for b in range(B):
        _check(fn + '.gbuf', inner[b, :, :wv[b]], want[b, :, :wv[b]], mag[b, :, :wv[b]], what='b=%d' % b)
        assert bool((inner[b, :, wv[b]:] == 0).all()), '%s: columns >= wvalid[%d] = %d are not zero' % (fn, b, wv[b])
    _border_is_zero(gb, p, fn)


def test_head_rejects_more_than_four_outputs():
    """nout = 5: the head's contract is nout <= 4 (mlp_bwd_kernel keeps dz3 in a 4-float LDS array), so the forward and the backward entry
    point must both return NELE_ERR_INVALID_ARG and write nothing.  The backward used to launch: its argument check had no nout."""
    L = _lib()
    B, Hout, Wout, p, nout = 2, 3, 5, 8, 5
    ws, bs, sg, host = _mlp(nout, 1)
    g = _gen(2)
    act = torch.randn((B, Hout, Wout, 64), device='cuda', generator=g)
    dscore, score = torch.randn((B, nout), device='cuda', generator=g), torch.rand((B, nout), device='cuda', generator=g)
    h1, h2 = torch.randn((B, 64), device='cuda', generator=g), torch.randn((B, 16), device='cuda', generator=g)
    outs = [_nan(B, nout), _nan(B, 16), _nan(B, 64), _nan(B, 64), _bordered(B, Hout, Wout, 64, p, NAN, torch.float32)]
    st = L.lib.nele_gap_mlp_bwd(L.ptr(dscore), L.ptr(score), L.ptr(h1), L.ptr(h2), L.ptr(act), host, nout, SLOPE, B, Hout, Wout, Hout + 2 * p, Wout + 2 * p,
                                p, p, *[L.ptr(t) for t in outs], L.stream())
    torch.cuda.synchronize()
    assert st == ERR_INVALID_ARG, st
    assert all(bool(torch.isnan(t[:, p:p + Hout, p:p + Wout] if t.dim() == 4 else t).all()) for t in outs), 'nele_gap_mlp_bwd rejected nout = 5 but wrote'
    fw = [_nan(B, 64), _nan(B, 64), _nan(B, 16), _nan(B, nout)]
    scratch = _nan(B, 32, 64, dtype=torch.float64)
    st = L.lib.nele_gap_mlp_fwd(L.ptr(act), B, Hout * Wout, host, nout, SLOPE, *[L.ptr(t) for t in fw], L.ptr(scratch), L.stream())
    torch.cuda.synchronize()
    assert st == ERR_INVALID_ARG and all(bool(torch.isnan(t).all()) for t in fw)


@pytest.mark.parametrize('B', cases.MLP_WGRAD_B)
def test_mlp_wgrad_both_rules(B):
    """nele_mlp_wgrad (dW = dz^T x, db = sum_b dz) at the head's three layers with B around the 8-wide batch loop and its tail: integer
    operands bit for bit, random operands by the S rule"""
    L = _lib()
    for N, K in cases.MLP_WGRAD_NK:
        for ints in (False, True):
            g = _gen(100 * B + N + int(ints))
            dz = _ints((B, N), cases.INT_W, g) if ints else torch.randn((B, N), device='cuda', generator=g)
            x = _ints((B, K), cases.INT_A, g) if ints else torch.randn((B, K), device='cuda', generator=g)
            dW, db = _nan(N * K + 8), _nan(N + 8)
            L.call('nele_mlp_wgrad', L.ptr(dz), L.ptr(x), B, N, K, L.ptr(dW), L.ptr(db), L.stream())
            torch.cuda.synchronize()
            rW, sW = dz.double().T @ x.double(), dz.double().abs().T @ x.double().abs()
            rb, sb = dz.double().sum(0), dz.double().abs().sum(0)
            if ints:
                assert float(sW.max()) < cases.LIMIT
                assert torch.equal(dW[:N * K].view(N, K), rW.float()) and torch.equal(db[:N], rb.float()), (B, N, K)
            else:
                _check('nele_mlp_wgrad', dW[:N * K].view(N, K), rW, sW, what='B=%d N=%d K=%d' % (B, N, K))
                _check('nele_mlp_wgrad.db', db[:N], rb, sb, what='B=%d N=%d' % (B, N))
            assert bool(torch.isnan(dW[N * K:]).all() and torch.isnan(db[N:]).all())


# ------------------------------------------------------------------------------------------ Adam
@pytest.mark.parametrize('n', [1, 255, 256 * 2048 + 5])
def test_adam_step_in_ulps(n):
    """nele_adam_step (and nele_adam_step_guarded with a zeroed guard: the same update), steps 1..3, each against float64 Adam on the float32
    state the kernel starts the step from (n = 256 * 2048 + 5 is beyond one grid-stride pass).  With b1, b2, lr, eps the float32 values the kernel receives (1 - b1 and 1 - b2 are exact in float32):
      m' = b1 m + (1 - b1) g: two products and a sum, half an ulp each:  |dm| <= ULP (|b1 m| + |(1 - b1) g|)
      v' = b2 v + (1 - b2) g g: three products and a sum, all terms positive:  |dv| <= 2 ULP v'
      p' = p - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps): sqrt halves v's relative error (1 ULP); sqrt, the quotient by float32(sqrt(bc2)), that
      constant and the sum with eps are half an ulp each (2 ULP); float32(bc1), lr / bc1, m' / denom and the product another 2 ULP; m' carries dm.
      So |dp| <= ULP / 2 |p'| (the final difference) + 5 ULP |update| + dm (lr / bc1) / denom, and |update| is of the order of lr:
      half an ulp of p plus a few 1e-7 of lr."""
    L = _lib()
    g = _gen(n % 1000)
    lr, b1, b2, eps = (float(np.float32(x)) for x in (2e-3, 0.9, 0.999, 1e-8))
    p = torch.randn(n, device='cuda', generator=g)
    m, v = torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
    guard = torch.zeros(2, dtype=torch.int32, device='cuda')
    for step in (1, 2, 3):
        grad = torch.randn(n, device='cuda', generator=g) * (10.0 ** torch.randint(-4, 2, (n,), device='cuda', generator=g).float())
        p0, m0, v0 = p.double(), m.double(), v.double()
        pg, mg, vg = p.clone(), m.clone(), v.clone()
        L.call('nele_adam_step', L.ptr(p), L.ptr(grad), L.ptr(m), L.ptr(v), n, lr, b1, b2, eps, step, L.stream())
        L.call('nele_adam_step_guarded', L.ptr(pg), L.ptr(grad), L.ptr(mg), L.ptr(vg), n, lr, b1, b2, eps, step, L.ptr(guard), L.stream())
        torch.cuda.synchronize()
        assert guard.tolist() == [0, 0], 'the guarded step counted a skipped step on finite gradients'
        pr, mr, vr, t = ref.adam_step(p0, grad.double(), m0, v0, lr, b1, b2, eps, step)
        dm = ULP * t['m_mag'] * (1 + 1e-6)                     # (the half ulp of the sum is of the rounded terms)
        what = 'n=%d step=%d' % (n, step)
        for fn, (pp, mm, vv) in (('nele_adam_step', (p, m, v)), ('nele_adam_step_guarded', (pg, mg, vg))):
            _bounded(fn + '.m', mm, mr, dm, what)
            _bounded(fn + '.v', vv, vr, 2 * ULP * t['v_mag'], what)
            _bounded(fn + '.p', pp, pr, 0.5 * ULP * pr.abs() + 5 * ULP * t['upd'].abs() + dm * t['gain'], what)
        assert float(t['upd'].abs().max()) <= 8 * lr


# ------------------------------------------------------------------------------------------ energy normalisation
def _energy_fwd(L, clean, mask, noise, want_din=True):
    B, T, _ = clean.shape
    beta2, s2 = _nan(B), _nan(B)
    din = _nan(B, 64, T, 4) if want_din else None
    alpha2 = _nan(B, T, 64)
    L.call('nele_energy_norm_fwd', L.ptr(clean), L.ptr(mask), L.ptr(noise), 1.0 / 6, 6.0, L.ptr(beta2), L.ptr(s2), L.ptr(din), L.ptr(alpha2), B, T, L.stream())
    torch.cuda.synchronize()
    return beta2, s2, din, alpha2


@pytest.mark.parametrize('T', [1, 63, 64, 65, 129, 501])
def test_energy_norm_forward(T):
    """nele_energy_norm_fwd with p = float32(1 / 6), inv_p = 6, B = 3, one utterance with trailing all-zero frames, at the edges of the
    64-frame tiles (T = 129: 8256 elements, the second pass of the eight-wide sum loop).  common.h promises clean^6 and x^p as the float32
    nearest to the true value, and the sums run in float64, so: s2 within 2^-24 relative of the float64 sum (test_prefix_norm_gpu.py's
    argument), beta2 within one ulp of S1 / S2, the enhanced band within 3 ulp of clean mask^p beta2^p (two powers, two products, on the
    kernel's own beta2), noise and clean copied bit for bit, channel 3 exactly 0, alpha2 = mask * beta2 in float32 bit for bit; with
    din = NULL, beta2 and alpha2 are bit-identical to the full call."""
    L = _lib()
    tail = (T, max(T // 2, 1), T)
    clean, mask, noise, _ = [torch.from_numpy(a).cuda() for a in ref.energy_inputs(3, T, 1000 + T, tail)]
    beta2, s2, din, alpha2 = _energy_fwd(L, clean, mask, noise)
    s1r, s2r = ref.energy_norm_sums(mask.double(), clean.double())
    _bounded('nele_energy_norm_fwd.s2', s2, s2r, 2.0 ** -24 * s2r, 'T=%d' % T)
    _bounded('nele_energy_norm_fwd.beta2', beta2, s1r / s2r, ULP * s1r / s2r, 'T=%d' % T)
    enh = clean.double() * mask.double() ** ref.P32 * (beta2.double() ** ref.P32)[:, None, None]
    _bounded('nele_energy_norm_fwd.enh', din[..., 0].permute(0, 2, 1), enh, 3 * ULP * enh + 1e-300, 'T=%d' % T)
    assert torch.equal(din[..., 1].permute(0, 2, 1), noise) and torch.equal(din[..., 2].permute(0, 2, 1), clean)
    assert bool((din[..., 3] == 0).all()) and not bool(torch.signbit(din[..., 3]).any())
    assert torch.equal(alpha2, mask * beta2[:, None, None])
    if T > 1:
        assert float(din[1, :, tail[1]:, :3].abs().max()) == 0.0
    b2, _, none, a2 = _energy_fwd(L, clean, mask, noise, want_din=False)
    assert none is None and torch.equal(b2, beta2) and torch.equal(a2, alpha2)


ENB_SHAPES = [(3, 57), (1, 129), (2, 501)]


def _enb_float32_cost(clean, mask, ddin):
    """worst error of the closed form evaluated in float32 torch on the CPU against float64, as a fraction of the peak"""
    c, m, dE = [torch.from_numpy(a) for a in (clean, mask, np.ascontiguousarray(ddin[..., 0].transpose(0, 2, 1)))]
    w64 = ref.energy_norm_dmask(m.double(), c.double(), dE.double())
    w32 = ref.energy_norm_dmask(m, c, dE, p=np.float32(1.0 / 6.0), inv_p=6)
    return float((w32.double() - w64).abs().max() / w64.abs().max()), w64


@pytest.mark.parametrize('with_din', [True, False])
@pytest.mark.parametrize('B,T', ENB_SHAPES)
def test_energy_norm_backward_against_the_closed_form(B, T, with_din):
    """dmask of nele_energy_norm_bwd (beta2 and s2 from the forward kernel, with and without its din) against the closed form in float64
    (glue_refs.energy_norm_dmask, held to float64 autograd of oracle.nets.energy_norm by test_glue_refs_cpu.py).  The bound is measured:
    the same closed form in float32 torch on the CPU on these inputs is off from float64 by 1.2e-7, 1.1e-7 and 1.6e-7 of the peak for the
    three shapes; the kernel is allowed 4 x that figure, recomputed here.  The kernel on the MI355X: 8.8e-8, 8.4e-8 and 9.0e-8 of the peak
    reading the forward pass's din, 1.2e-7, 1.8e-7 and 1.8e-7 recomputing the enhanced band (at most 1.65 x the float32 figure)."""
    L = _lib()
    arrs = ref.energy_inputs(B, T, 11 * B + T)
    cost32, want = _enb_float32_cost(arrs[0], arrs[1], arrs[3])
    clean, mask, noise, ddin = [torch.from_numpy(a).cuda() for a in arrs]
    beta2, s2, din, _ = _energy_fwd(L, clean, mask, noise)
    dmask = _nan(B, T, 64)
    L.call('nele_energy_norm_bwd', L.ptr(clean), L.ptr(mask), L.ptr(beta2), L.ptr(s2), L.ptr(ddin), L.ptr(din if with_din else None), 1.0 / 6, 6.0,
           L.ptr(dmask), B, T, L.stream())
    torch.cuda.synchronize()
    err = float((dmask.double().cpu() - want).abs().max() / want.abs().max())
    print('nele_energy_norm_bwd B %d T %d din %s: %.3e of peak; float32 closed form on the CPU: %.3e' % (B, T, with_din, err, cost32))
    key = 'nele_energy_norm_bwd.%s/float32_cost' % ('din' if with_din else 'recomputed')
    MARGINS[key] = max(MARGINS.get(key, 0.0), err / cost32)
    assert err <= 4 * cost32, (err, cost32)


# ------------------------------------------------------------------------------------------ exp(3.2 tanh) gradient
def test_exptanh_backward_over_the_whole_mask_range():
    """nele_exptanh_bwd: dmask m 3.2 (1 - th^2), th = ln(m) / 3.2, for masks m = float32(exp(3.2 tanh(x))), x in [-6, 6] (near saturation
    1 - th^2 cancels), n no multiple of the 256-thread block.  Reference: float64 on the same float32 mask.  th is logf(m) * float32(1 / 3.2):
    logf within 1 ulp (HIP's documented bound), the constant and the product half an ulp each, so |dth| <= 2 ULP |th| = delta; th * th adds
    half an ulp of th^2.  Through 1 - th^2 that is an ABSOLUTE error |dmask| m 3.2 (2 |th| delta + ULP / 2 th^2); the difference, the three
    products and float32(3.2) add 3 ULP of the result."""
    L = _lib()
    n = 5 * 256 + 77
    g = _gen(3)
    x = torch.cat([torch.linspace(-6, 6, n - 200, device='cuda', dtype=torch.float64), 6 * torch.rand(200, device='cuda', generator=g).double() - 3])
    mask = torch.exp(3.2 * torch.tanh(x)).float()
    dmask = torch.randn(n, device='cuda', generator=g)
    dout = _nan(n + 8)
    L.call('nele_exptanh_bwd', L.ptr(dmask), L.ptr(mask), L.ptr(dout), n, L.stream())
    torch.cuda.synchronize()
    m64, d64 = mask.double(), dmask.double()
    th = torch.log(m64) / 3.2
    want = d64 * m64 * 3.2 * (1 - th * th)
    delta = 2 * ULP * th.abs()
    bound = d64.abs() * m64 * 3.2 * (2 * th.abs() * delta + 0.5 * ULP * th * th) + 3 * ULP * want.abs()
    assert float(th.abs().max()) > 0.9999 and float(th.abs().min()) < 1e-3          # the whole range, saturation included
    _bounded('nele_exptanh_bwd', dout[:n], want, bound)
    assert bool(torch.isnan(dout[n:]).all())


# ------------------------------------------------------------------------------------------ column sums and layouts
@pytest.mark.parametrize('rows,cols', cases.COLSUM_SHAPES)
def test_colsum_integer_rule(rows, cols):
    """nele_colsum on integers {-4..4}, accumulate 0 into NaN and 1 onto integers: bit for bit (sums below 2^24); around the 16 row groups
    and the 64-column blocks, nothing written behind the last column"""
    L = _lib()
    g = _gen(rows * 1000 + cols)
    part = _ints((rows, cols), cases.INT_A, g)
    want = part.double().sum(0)
    assert float(part.abs().sum(0).max()) + cases.INT_A < cases.LIMIT
    for acc in (0, 1):
        out = _nan(cols + 8)
        old = _ints((cols,), cases.INT_A, g)
        if acc:
            out[:cols] = old
        L.call('nele_colsum', L.ptr(part), rows, cols, L.ptr(out), acc, L.stream())
        torch.cuda.synchronize()
        assert torch.equal(out[:cols], (want + (old.double() if acc else 0)).float()), (rows, cols, acc)
        assert bool(torch.isnan(out[cols:]).all())


@pytest.mark.parametrize('T', [1, 63, 65])
def test_pack_and_layout_kernels_are_torch_indexing(T):
    """nele_g_pack, nele_d_pack (with and without c2) and nele_d_layout in both directions (Cin = 2, 3): bit-equal to torch indexing; the
    fourth channel and the channels >= Cin exactly zero; nele_g_pack writes the rows pad.. only (the padding rows of a zeroed buffer stay
    zero, of a NaN buffer NaN: zeroing them once is the caller's job); NHWC -> NCHW -> NHWC is the identity."""
    L = _lib()
    B, pad = 3, 4
    g = _gen(T)
    x, y, c2 = (torch.randn((B, T, 64), device='cuda', generator=g) for _ in range(3))
    for fill in (0.0, NAN):
        out = torch.full((B, T + pad, 128), fill, device='cuda')
        L.call('nele_g_pack', L.ptr(x), L.ptr(y), L.ptr(out), B, T, pad, L.stream())
        torch.cuda.synchronize()
        assert torch.equal(out[:, pad:], torch.cat((x, y), 2))
        assert bool((out[:, :pad] == 0).all() if fill == 0.0 else torch.isnan(out[:, :pad]).all())
    for third in (c2, None):
        din = _nan(B, 64, T, 4)
        L.call('nele_d_pack', L.ptr(x), L.ptr(y), L.ptr(third), L.ptr(din), B, T, L.stream())
        torch.cuda.synchronize()
        assert torch.equal(din[..., 0], x.transpose(1, 2)) and torch.equal(din[..., 1], y.transpose(1, 2))
        assert torch.equal(din[..., 2], c2.transpose(1, 2)) if third is not None else bool((din[..., 2] == 0).all())
        assert bool((din[..., 3] == 0).all())
    for Cin in (2, 3):
        src = torch.randn((B, Cin, 64, T), device='cuda', generator=g)
        nhwc = _nan(B, 64, T, 4)
        L.call('nele_d_layout', L.ptr(src), L.ptr(nhwc), B, Cin, T, 1, L.stream())
        torch.cuda.synchronize()
        assert torch.equal(nhwc[..., :Cin], src.permute(0, 2, 3, 1)) and bool((nhwc[..., Cin:] == 0).all())
        back = _nan(B, Cin, 64, T)
        L.call('nele_d_layout', L.ptr(nhwc), L.ptr(back), B, Cin, T, 0, L.stream())
        torch.cuda.synchronize()
        assert torch.equal(back, src)
        again = _nan(B, 64, T, 4)
        L.call('nele_d_layout', L.ptr(back), L.ptr(again), B, Cin, T, 1, L.stream())
        torch.cuda.synchronize()
        assert torch.equal(again, nhwc)
