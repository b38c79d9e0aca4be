"""GPU: the bf16 kernels of the discriminator and of the generator's backward against float64 on the operands they actually multiply.

Every reference below runs in float64 on the SAME bf16-rounded values the kernel reads (torch's float -> bfloat16 conversion is RNE, as
the kernels' __bf16 conversion).  The only legitimate difference is then the float32 accumulation order, plus one bf16 rounding where a
result is stored as bf16.  With S = sum |a * w| (the same operation on absolute values), per element:

  * float32 outputs:  |got - ref| <= 2e-5 S
  * bf16 outputs:     |got - ref| <= 2e-5 S + 2^-8 |ref|

Output buffers start as NaN sentinels; what the contract says is not written must still be the sentinel, or still zero where the contract
says a border stays zero.  These checks run in seconds and are ~1000 x tighter than the end-to-end bf16 tests: a rewrite of conv16.hip,
of dense.hip's bf16 paths or of gen.hip's cLN must pass them.  The largest measured |got - ref| / S per kernel is written as JSON to
$NELE_EXACT_MARGINS when that variable is set.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from exact_rules import (C32, D_CONVS, EPI_BIAS, EPI_BIAS_LRELU, EPI_MASK_LRELU_GRAD, EPI_NONE, ERR_UNSUPPORTED, G_LAYERS, MARGINS, P_,  # noqa: E402,F401
                         SLOPE, _border_is_zero, _bordered, _check, _conv, _d_dims, _flip_layout, _flip_weight, _fwd_layout, _gen, _geom,
                         _head_ref, _lib, _lrelu, _mlp, _r16, _report_margins, _wgrad_ref)

# (B, T): T = 52 is the shortest that takes the conv16 path; the others leave partial 64-column and 4- / 8-row tiles at every layer
NET_BT = [(1, 52), (2, 53), (3, 64), (1, 85), (2, 117), (3, 149), (1, 251)]


# ------------------------------------------------------------------------------------------ helpers
def _frag16(L, Wg, N, C, KH, KW):
    """conv16 fragment stream of a GEMM-layout weight Wg [N][KH * KW * C] float32"""
    wf = torch.empty(int(L.lib.nele_conv16_wfrag_elems(N, KW * C, KH)), dtype=torch.bfloat16, device='cuda')
    L.call('nele_conv16_weight_prep_batch', (P_ * 2)(Wg.data_ptr(), wf.data_ptr()), (ctypes.c_int * 4)(N, KH * KW * C, KW * C, KH), 1, L.stream())
    return wf


def _rand_conv(B, H, W, C, N, KH, KW, seed, bias_scale=0.1):
    g = _gen(seed)
    A = torch.randn((B, H, W, C), device='cuda', generator=g).to(torch.bfloat16)
    Wt = _r16(torch.randn((N, C, KH, KW), device='cuda', generator=g) / np.sqrt(C * KH * KW))
    bias = bias_scale * torch.randn(N, device='cuda', generator=g)
    return A, Wt, bias


# ------------------------------------------------------------------------------------------ 1. kernels at the network's geometries
@pytest.mark.parametrize('B,T', NET_BT)
def test_conv16_forward_at_the_discriminator_layers(B, T):
    """nele_conv16 forward of D.conv2-4 (EPI_BIAS_LRELU, bf16 and float32 stores) at the geometries netplan.hip d_layout builds, plus EPI_NONE and
    EPI_BIAS once.  Tolerance: the rule of the module docstring (float32 accumulation of up to 48 * 49 products; one bf16 rounding)."""
    L = _lib()
    dims = _d_dims(T)
    for l in (1, 2, 3):
        (Hi, Wi, Ci), (Ho, Wo, co), k = dims[l], dims[l + 1], D_CONVS[l][1]
        A, Wt, bias = _rand_conv(B, Hi, Wi, Ci, co, k, k, 100 * T + 10 * B + l)
        geom = _geom(Hi, Wi, Ci, Ho, Wo, k, k, Ho, Wo, co)
        assert L.lib.nele_conv16_supported(B * Ho * Wo, co, geom, k, k) == 1
        wf = _frag16(L, _fwd_layout(Wt), co, Ci, k, k)
        raw, S = _conv(A, Wt)
        ref, Sb = _lrelu(raw + bias.double()), S + bias.double().abs()
        epis = [(EPI_BIAS_LRELU, ref, Sb)]
        if (B, T) == NET_BT[0]:
            epis += [(EPI_NONE, raw, S), (EPI_BIAS, raw + bias.double(), Sb)]
        for epi, r, s in epis:
            for out16 in ((1, 0) if epi == EPI_BIAS_LRELU else (0,)):
                out = torch.full((B, Ho, Wo, co), float('nan'), device='cuda', dtype=torch.bfloat16 if out16 else torch.float32)
                L.call('nele_conv16', L.ptr(A), L.ptr(wf), L.ptr(bias), None, L.ptr(out), out16, B * Ho * Wo, co, epi, SLOPE, geom, k, k, L.stream())
                torch.cuda.synchronize()
                _check('nele_conv16.fwd', out, r, s, bf16_out=bool(out16), what='D.conv%d B=%d T=%d epi=%d out16=%d' % (l + 1, B, T, epi, out16))


@pytest.mark.parametrize('B,T', NET_BT)
def test_conv16_data_gradient_at_the_discriminator_layers(B, T):
    """nele_conv16 data gradient of D.conv2-5 (EPI_MASK_LRELU_GRAD): the flipped-weight convolution over the zero-bordered gbuf[l], gated by
    the stored bf16 forward activation (derivative act > 0 ? 1 : slope), written into the bordered gbuf[l-1] (float32 for l = 1, as in the
    network) whose border must stay exactly zero.  Tolerance: the rule (up to 64 * 81 products)."""
    L = _lib()
    dims = _d_dims(T)
    for l in (1, 2, 3, 4):
        (Hi, Wi, Ci), (Ho, Wo, co), k = dims[l], dims[l + 1], D_CONVS[l][1]
        p, pp = k - 1, D_CONVS[l - 1][1] - 1
        g = _gen(200 * T + 10 * B + l)
        gin = _bordered(B, Ho, Wo, co, p, torch.randn((B, Ho, Wo, co), device='cuda', generator=g).to(torch.bfloat16), torch.bfloat16)
        act = torch.randn((B, Hi, Wi, Ci), device='cuda', generator=g).to(torch.bfloat16)
        Wt = _r16(torch.randn((co, Ci, k, k), device='cuda', generator=g) / np.sqrt(co * k * k))
        geom = _geom(Ho + 2 * p, Wo + 2 * p, co, Hi, Wi, k, k, Hi + 2 * pp, Wi + 2 * pp, Ci, 0, 0, pp, pp)
        assert L.lib.nele_conv16_supported(B * Hi * Wi, Ci, geom, k, k) == 1
        wf = _frag16(L, _flip_layout(Wt), Ci, co, k, k)
        out16 = 1 if l >= 2 else 0
        out = _bordered(B, Hi, Wi, Ci, pp, float('nan'), torch.bfloat16 if out16 else torch.float32)
        L.call('nele_conv16', L.ptr(gin), L.ptr(wf), None, L.ptr(act), L.ptr(out), out16, B * Hi * Wi, Ci, EPI_MASK_LRELU_GRAD, SLOPE, geom, k, k, L.stream())
        torch.cuda.synchronize()
        raw, S = _conv(gin, _flip_weight(Wt))
        m = torch.where(act.double() > 0, 1.0, SLOPE)
        _check('nele_conv16.dgrad', out[:, pp:pp + Hi, pp:pp + Wi], raw * m, S * m, bf16_out=bool(out16), what='D.conv%d B=%d T=%d' % (l + 1, B, T))
        _border_is_zero(out, pp, 'nele_conv16.dgrad D.conv%d' % (l + 1))


@pytest.mark.parametrize('B,T', NET_BT)
def test_conv16_gap_and_the_head_on_its_partial_sums(B, T):
    """nele_conv16_gap (D.conv5 with the pooling fused): out16 by the rule; the float64 sum of the gap_part partial sums against the float64
    sum of LeakyReLU(conv + bias) over the columns < wvalid[b] (wvalid NULL, and one value per row, one of them 1), within 2e-5 of the summed S;
    then nele_gap_mlp_fwd_parts on those partials against a float64 head: pooled to 1e-6 (one float32 rounding of the mean), h1 / h2 / score
    within 2e-5 of their propagated magnitudes (float32 dot products of 64 / 16 terms)."""
    L = _lib()
    dims = _d_dims(T)
    (Hi, Wi, Ci), (Ho, Wo, co), k = dims[4], dims[5], 9
    A, Wt, bias = _rand_conv(B, Hi, Wi, Ci, co, k, k, 300 * T + B)
    A = (A.float() + 0.05).to(torch.bfloat16)                 # (positive-leaning activations: the pooled means are not all ~0)
    geom = _geom(Hi, Wi, Ci, Ho, Wo, k, k, Ho, Wo, co)
    parts = L.lib.nele_conv16_gap_parts(co, geom, k, k)
    assert parts > 0
    wf = _frag16(L, _fwd_layout(Wt), co, Ci, k, k)
    raw, S = _conv(A, Wt)
    ref, Sb = _lrelu(raw + bias.double()), S + bias.double().abs()
    ws, bs, sg, host = _mlp(3, 7 * T + B)
    for wv in (None, [1, Wo - 7, (2 * Wo) // 3][:B]):
        wvt = None if wv is None else torch.tensor(wv, dtype=torch.int32, device='cuda')
        cols = [Wo] * B if wv is None else wv
        out16 = torch.full((B, Ho, Wo, co), float('nan'), dtype=torch.bfloat16, device='cuda')
        gap = torch.full((B, parts, co), float('nan'), dtype=torch.float64, device='cuda')
        L.call('nele_conv16_gap', L.ptr(A), L.ptr(wf), L.ptr(bias), L.ptr(out16), B * Ho * Wo, co, SLOPE, geom, k, k, L.ptr(wvt), L.ptr(gap), L.stream())
        torch.cuda.synchronize()
        _check('nele_conv16_gap.out16', out16, ref, Sb, bf16_out=True, what='B=%d T=%d' % (B, T))
        assert bool(torch.isfinite(gap).all()), 'nele_conv16_gap: a partial sum was not written'
        tot = gap.sum(1)
        rsum = torch.stack([ref[b, :, :cols[b]].sum((0, 1)) for b in range(B)])
        ssum = torch.stack([Sb[b, :, :cols[b]].sum((0, 1)) for b in range(B)])
        _check('nele_conv16_gap.parts', tot, rsum, ssum, what='B=%d T=%d wvalid=%s' % (B, T, wv))
        # the head on those partials
        pooled, h1, h2 = (torch.full((B, n), float('nan'), device='cuda') for n in (64, 64, 16))
        score = torch.full((B, 3), float('nan'), device='cuda')
        L.call('nele_gap_mlp_fwd_parts', L.ptr(gap), parts, B, Ho * Wo, Wo, L.ptr(wvt), host, 3, SLOPE, L.ptr(pooled), L.ptr(h1), L.ptr(h2), L.ptr(score), L.stream())
        torch.cuda.synchronize()
        pref = tot / torch.tensor([Ho * c for c in cols], dtype=torch.float64, device='cuda')[:, None]
        _check('nele_gap_mlp_fwd_parts.pooled', pooled, pref, pref.abs(), c=1e-6)
        for name, got, (r, s) in zip(('h1', 'h2', 'score'), (h1, h2, score), _head_ref(pooled, ws, bs, sg)):
            _check('nele_gap_mlp_fwd_parts.' + name, got, r, s, what='B=%d T=%d' % (B, T))


@pytest.mark.parametrize('B,T', [(1, 52), (3, 149)])
def test_conv16_pointwise_is_float32_exact(B, T):
    """nele_conv16_pointwise_fwd (D.layers.0, 1 x 1, 4 -> 8 channels): float32-exact arithmetic of 4 products + bias + LeakyReLU, so out16 must
    be bf16(float64 result) up to one bf16 step (the float32 result can sit on the other side of a rounding boundary)."""
    L = _lib()
    g = _gen(T + B)
    M = B * 64 * T
    x = torch.randn((M, 4), device='cuda', generator=g)
    Wf = torch.randn((8, 4), device='cuda', generator=g)
    bias = 0.1 * torch.randn(8, device='cuda', generator=g)
    out = torch.full((M, 8), float('nan'), dtype=torch.bfloat16, device='cuda')
    L.call('nele_conv16_pointwise_fwd', L.ptr(x), L.ptr(Wf), L.ptr(bias), L.ptr(out), M, 8, SLOPE, L.stream())
    torch.cuda.synchronize()
    ref = _lrelu(x.double() @ Wf.double().T + bias.double())
    r16 = ref.to(torch.bfloat16)
    steps = (out.view(torch.int16).int() - r16.view(torch.int16).int()).abs()
    same_sign = (out.float() >= 0) == (r16.float() >= 0)
    ok = (steps <= 1) & same_sign | (out.double() - ref).abs().le(1e-30)
    assert bool(ok.all()), 'nele_conv16_pointwise_fwd: %d elements more than one bf16 step from the float64 result' % int((~ok).sum())
    MARGINS['nele_conv16_pointwise_fwd.bf16_steps'] = max(MARGINS.get('nele_conv16_pointwise_fwd.bf16_steps', 0), int(steps.max()))


@pytest.mark.parametrize('B,T,act16', [(1, 52, True), (3, 149, True), (2, 53, False), (3, 85, False)])
def test_head_backward_and_the_bf16_pooling_gradient(B, T, act16):
    """nele_gap_mlp_bwd_var16a (bf16 activation) and nele_gap_mlp_bwd_var16 (float32 activation) against float64 autograd of the head:
    dz3 / dz2 / dz1 / dpooled within 2e-5 of their propagated magnitudes; the bf16 pooling gradient dpooled / (Hout * wvalid) * LeakyReLU'(act)
    by the bf16 rule, exactly zero at columns >= wvalid[b] and on the border of the bordered buffer."""
    L = _lib()
    g = _gen(17 * T + B)
    Ho, Wo, p, nout = 44, T - 20, 8, 3
    ws, bs, sg, host = _mlp(nout, 5 * T + B)
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
    act = torch.randn((B, Ho, Wo, 64), device='cuda', generator=g)
    act = act.to(torch.bfloat16) if act16 else act
    wv = [Wo, 1, Wo - 5][:B] if B > 1 else [Wo - 3]
    wvt = torch.tensor(wv, dtype=torch.int32, device='cuda')
    dz3, dz2, dz1, dp = (torch.full((B, n), float('nan'), device='cuda') for n in (nout, 16, 64, 64))
    gb = _bordered(B, Ho, Wo, 64, p, float('nan'), torch.bfloat16)
    fn = 'nele_gap_mlp_bwd_var16a' if act16 else 'nele_gap_mlp_bwd_var16'
    L.call(fn, L.ptr(dscore), L.ptr(score), L.ptr(h1), L.ptr(h2), L.ptr(act), host, nout, SLOPE, B, Ho, Wo, L.ptr(wvt), Ho + 2 * p, Wo + 2 * p, p, p,
           L.ptr(dz3), L.ptr(dz2), L.ptr(dz1), L.ptr(dp), L.ptr(gb), L.stream())
    torch.cuda.synchronize()
    s = (dscore.double() * score.double() * (1 - score.double())).abs()
    for q, (name, got) in enumerate((('dz3', dz3), ('dz2', dz2), ('dz1', dz1))):
        _check(fn + '.' + name, got, zs[2 - q].grad, s)
        w = (ws[2 - q].double() / sg[2 - q].double()).abs()
        s = (s @ w) * (1.0 if q == 2 else torch.where(zs[1 - q].detach() > 0, 1.0, SLOPE))
    _check(fn + '.dpooled', dp, pooled.grad, s)
    m = torch.where(act.double() > 0, 1.0, SLOPE)
    inner = gb[:, p:p + Ho, p:p + Wo].double()
    for b in range(B):
        n = Ho * wv[b]
        _check(fn + '.gbuf16', inner[b, :, :wv[b]], pooled.grad[b] / n * m[b, :, :wv[b]], s[b] / n * m[b, :, :wv[b]], bf16_out=True)
        assert bool((inner[b, :, wv[b]:] == 0).all()), '%s: columns >= wvalid[%d] = %d are not zero' % (fn, b, wv[b])
    _border_is_zero(gb, p, fn)


def _wgrad_call(L, fn, A, dO, geom, M, N, KH, KW, Cvalid, dW, db, accumulate):
    nws = int(L.lib.nele_conv_wgrad_workspace_floats(M, N, KH * KW * A.shape[-1], None))
    wsb = torch.empty(nws, device='cuda')
    L.call(fn, L.ptr(A), L.ptr(dO), L.ptr(wsb), nws, M, N, geom, KH, KW, Cvalid, L.ptr(dW), L.ptr(db), accumulate, L.stream())
    torch.cuda.synchronize()


def _wgrad_all_entries(L, tag, A16, dObuf16, dOin, geom, M, N, KH, KW, Cvalid, seed):
    """the three bf16 weight-gradient entry points on one geometry: a16d16 (accumulate 0 into NaN, then 1 onto random values), d16, bf16.
    dObuf16: the output-gradient buffer the geometry addresses (bf16); dOin: its region of the output positions [B][Hout][Wout][N]."""
    C = A16.shape[-1]
    rW, sW = _wgrad_ref(A16[..., :Cvalid], dOin, (N, Cvalid, KH, KW))
    rb, sb = dOin.double().sum((0, 1, 2)), dOin.double().abs().sum((0, 1, 2))
    g = _gen(seed)
    nW = N * Cvalid * KH * KW
    for fn, a, d in (('nele_conv_wgrad_bf16_a16d16', A16, dObuf16), ('nele_conv_wgrad_bf16_d16', A16.float(), dObuf16),
                     ('nele_conv_wgrad_bf16', A16.float(), dObuf16.float())):
        if fn.endswith('_d16') and not L.lib.nele_conv_wgrad_bf16_d16_supported(M, N, geom, KH, KW):
            # (G's layers: the float32-activation form only runs on the 2-D tile kernel, which declines them; G passes bf16 activations)
            dWbuf = torch.full((nW,), float('nan'), device='cuda')
            nws = int(L.lib.nele_conv_wgrad_workspace_floats(M, N, KH * KW * C, None))
            wsb = torch.empty(nws, device='cuda')
            assert L.lib.nele_conv_wgrad_bf16_d16(L.ptr(a), L.ptr(d), L.ptr(wsb), nws, M, N, geom, KH, KW, Cvalid, L.ptr(dWbuf), None, 0, L.stream()) == ERR_UNSUPPORTED
            torch.cuda.synchronize()
            assert bool(torch.isnan(dWbuf).all()), '%s declined %s but wrote dW' % (fn, tag)
            continue
        for acc in ((0, 1) if fn.endswith('a16d16') else (0,)):
            dWbuf = torch.full((nW + 64,), float('nan'), device='cuda')
            dbbuf = torch.full((N + 4,), float('nan'), device='cuda')
            base_w = base_b = 0
            if acc:
                base_w, base_b = torch.randn(nW, device='cuda', generator=g), torch.randn(N, device='cuda', generator=g)
                dWbuf[:nW], dbbuf[:N] = base_w, base_b
                base_w, base_b = base_w.double(), base_b.double()
            _wgrad_call(L, fn, a, d, geom, M, N, KH, KW, Cvalid, dWbuf, dbbuf, acc)
            what = '%s accumulate=%d' % (tag, acc)
            _check(fn, dWbuf[:nW].view(N, Cvalid, KH, KW), rW + (base_w.view(N, Cvalid, KH, KW) if acc else 0),
                   sW + (2 ** -23 / C32) * (base_w.abs().view(N, Cvalid, KH, KW) if acc else 0), what=what)
            _check(fn + '.db', dbbuf[:N], rb + base_b, sb + (2 ** -23 / C32) * (base_b.abs() if acc else 0), what=what)
            assert bool(torch.isnan(dWbuf[nW:]).all() and torch.isnan(dbbuf[N:]).all()), '%s: wrote past dW / db' % fn


@pytest.mark.parametrize('B,T', NET_BT[::2])
def test_bf16_weight_gradients_at_the_network_layers(B, T):
    """nele_conv_wgrad_bf16_a16d16 / _d16 / nele_conv_wgrad_bf16 at D.conv2-5 (the gw geometries: dOut read from the zero-bordered gradient
    buffer) and at G's Conv1d layers (END-padded dY16 as g_backward passes it), against conv2d_weight and sum(dOut) in float64.  accumulate = 1
    adds to random values (allowance: one float32 rounding of the sum).  Tolerance: the rule; the sums run over up to 3 * 44 * 231 positions."""
    L = _lib()
    dims = _d_dims(T)
    for l in (1, 2, 3, 4):
        (Hi, Wi, Ci), (Ho, Wo, co), k = dims[l], dims[l + 1], D_CONVS[l][1]
        p = k - 1
        g = _gen(400 * T + 10 * B + l)
        A16 = torch.randn((B, Hi, Wi, Ci), device='cuda', generator=g).to(torch.bfloat16)
        dOin = (0.1 * torch.randn((B, Ho, Wo, co), device='cuda', generator=g)).to(torch.bfloat16)
        dO = _bordered(B, Ho, Wo, co, p, dOin, torch.bfloat16)
        geom = _geom(Hi, Wi, Ci, Ho, Wo, k, k, Ho + 2 * p, Wo + 2 * p, co, 0, 0, p, p)
        _wgrad_all_entries(L, 'D.conv%d B=%d T=%d' % (l + 1, B, T), A16, dO, dOin, geom, B * Ho * Wo, co, k, k, Ci, 11 * l + T)
    for q, (cin, cout, K) in enumerate(G_LAYERS):
        g = _gen(500 * T + 10 * B + q)
        A16 = torch.zeros((B, 1, T + K - 1, cin), dtype=torch.bfloat16, device='cuda')
        A16[:, :, K - 1:] = torch.randn((B, 1, T, cin), device='cuda', generator=g).to(torch.bfloat16)
        dOin = (0.1 * torch.randn((B, 1, T, cout), device='cuda', generator=g)).to(torch.bfloat16)
        dO = torch.zeros((B, 1, T + K - 1, cout), dtype=torch.bfloat16, device='cuda')
        dO[:, :, :T] = dOin
        geom = _geom(1, T + K - 1, cin, 1, T, 1, K, 1, T + K - 1, cout)
        _wgrad_all_entries(L, 'G %dx%dx%d B=%d T=%d' % (cin, cout, K, B, T), A16, dO, dOin, geom, B * T, cout, 1, K, cin, 13 * q + T)


def test_bf16_weight_gradients_with_fewer_valid_input_channels():
    """Cvalid < C on the bf16 weight-gradient entry points (the network passes it to the float32 kernel only, for D.layers.0's 3 of 4
    channels, but the ABI accepts it): C = 8, Cvalid = 5, 3 x 3 and 5 x 3 kernels; the channels >= Cvalid hold large values that must not leak
    in, and dW [N][Cvalid][KH][KW] must not be written past its end."""
    L = _lib()
    for q, (B, Hi, Wi, N, KH, KW) in enumerate(((2, 12, 70, 16, 3, 3), (1, 9, 100, 8, 5, 3))):
        g = _gen(900 + q)
        A16 = torch.randn((B, Hi, Wi, 8), device='cuda', generator=g)
        A16[..., 5:] = 1e4
        A16 = A16.to(torch.bfloat16)
        Ho, Wo = Hi - KH + 1, Wi - KW + 1
        dOin = torch.randn((B, Ho, Wo, N), device='cuda', generator=g).to(torch.bfloat16)
        geom = _geom(Hi, Wi, 8, Ho, Wo, KH, KW, Ho, Wo, N)
        _wgrad_all_entries(L, 'C=8 Cvalid=5 %dx%d' % (KH, KW), A16, dOin.contiguous(), dOin, geom, B * Ho * Wo, N, KH, KW, 5, 77 + q)


@pytest.mark.parametrize('B,T', [(1, 117), (3, 149), (2, 251)])
def test_span_bf16_a16_data_gradient_of_the_last_layer(B, T):
    """nele_conv_span_bf16_a16: D.conv5's data gradient from the bf16 pooling gradient into the bordered float32 gbuf[3], gated by the float32
    activation; the border stays zero.  Tolerance: the rule (64 * 81 products).  The span kernel takes this geometry from T = 117 on (rows of
    >= 64 output columns); D plans it where conv16 is switched off (NELE_D_CONV16=0), and at T < 52 the geometry is declined."""
    L = _lib()
    dims = _d_dims(T)
    (Hi, Wi, Ci), (Ho, Wo, co), k = dims[4], dims[5], 9
    p, pp = 8, 6
    g = _gen(600 + 10 * B + T)
    gin = _bordered(B, Ho, Wo, co, p, torch.randn((B, Ho, Wo, co), device='cuda', generator=g).to(torch.bfloat16), torch.bfloat16)
    act = torch.randn((B, Hi, Wi, Ci), device='cuda', generator=g)
    Wt = _r16(torch.randn((co, Ci, k, k), device='cuda', generator=g) / np.sqrt(co * k * k))
    geom = _geom(Ho + 2 * p, Wo + 2 * p, co, Hi, Wi, k, k, Hi + 2 * pp, Wi + 2 * pp, Ci, 0, 0, pp, pp)
    M = B * Hi * Wi
    assert L.lib.nele_conv_span_bf16_a16_supported(M, Ci, geom, k, k) == 1
    Wb = _flip_layout(Wt)
    wf = torch.empty(int(L.lib.nele_weight_frag16_elems(Ci, k * co, k)), dtype=torch.bfloat16, device='cuda')
    L.call('nele_weight_prep_frag16', L.ptr(Wb), Ci, Wb.shape[1], k * co, k, L.ptr(wf), L.stream())
    out = _bordered(B, Hi, Wi, Ci, pp, float('nan'), torch.float32)
    L.call('nele_conv_span_bf16_a16', L.ptr(gin), L.ptr(wf), None, L.ptr(act), L.ptr(out), M, Ci, EPI_MASK_LRELU_GRAD, SLOPE, geom, k, k, gin.numel(), L.stream())
    torch.cuda.synchronize()
    raw, S = _conv(gin, _flip_weight(Wt))
    m = torch.where(act.double() > 0, 1.0, SLOPE)
    _check('nele_conv_span_bf16_a16', out[:, pp:pp + Hi, pp:pp + Wi], raw * m, S * m, what='B=%d T=%d' % (B, T))
    _border_is_zero(out, pp, 'nele_conv_span_bf16_a16')


def _cln_call_bufs(B, T, C, pad, pade, chunks):
    nan = float('nan')
    return dict(out=torch.full((B, T + pad, C), nan, device='cuda'), mean=torch.full((B, T), nan, device='cuda'), rstd=torch.full((B, T), nan, device='cuda'),
                dY=torch.full((B, T + pade, C), nan, device='cuda'), dY16=torch.full((B, T + pade, C), nan, dtype=torch.bfloat16, device='cuda'),
                gp=torch.full((B * chunks, C), nan, device='cuda'), bp=torch.full((B * chunks, C), nan, device='cuda'),
                scratch=torch.empty((B, T, 2), dtype=torch.float64, device='cuda'))


@pytest.mark.parametrize('T,C', [(1, 256), (15, 256), (16, 256), (17, 64), (251, 256), (1024, 256)])
def test_cln_forward_and_backward_against_float64_autograd(T, C):
    """nele_cln_fwd / nele_cln_bwd (+ nele_colsum2 on the gain / bias partials) against float64 autograd of oracle/nets.py cln + LeakyReLU:
    mean / rstd to 1e-6 (float64 statistics rounded once to float32); the activation, dY and the reduced gain / bias gradients within 2e-5 of
    their magnitude sums (float32 arithmetic, float64 suffix sums); dY16 by the bf16 rule.  The END padding of dY / dY16 and the rows before
    `pad` of the activation are not written.  T = 1 .. 1024 = CLN_MAX_T, around the 16-frame chunks (CLN_FR)."""
    from oracle.nets import cln
    L = _lib()
    B, pad, pade = 2, 4, 6
    g = _gen(T * 7 + C)
    Y = 0.5 + torch.randn((B, T, C), device='cuda', generator=g)
    gain = 1 + 0.2 * torch.randn(C, device='cuda', generator=g)
    beta = 0.1 * torch.randn(C, device='cuda', generator=g)
    dAct = torch.randn((B, T, C), device='cuda', generator=g)
    chunks = L.lib.nele_cln_chunks(T)
    bf = _cln_call_bufs(B, T, C, pad, pade, chunks)
    s = L.stream()
    L.call('nele_cln_fwd', L.ptr(Y), L.ptr(gain), L.ptr(beta), L.ptr(bf['out']), L.ptr(bf['mean']), L.ptr(bf['rstd']), L.ptr(bf['scratch']), B, T, C, pad, SLOPE, s)
    L.call('nele_cln_bwd', L.ptr(dAct), L.ptr(Y), L.ptr(gain), L.ptr(beta), L.ptr(bf['mean']), L.ptr(bf['rstd']), L.ptr(bf['dY']), L.ptr(bf['dY16']), L.ptr(bf['gp']),
           L.ptr(bf['bp']), L.ptr(bf['scratch']), B, T, C, pade, SLOPE, s)
    dg, db = torch.full((C,), float('nan'), device='cuda'), torch.full((C,), float('nan'), device='cuda')
    L.call('nele_colsum2', L.ptr(bf['gp']), L.ptr(dg), L.ptr(bf['bp']), L.ptr(db), B * chunks, C, 0, s)
    torch.cuda.synchronize()
    bf = {k: v.cpu() for k, v in bf.items()}
    dg, db = dg.cpu(), db.cpu()
    # float64 reference on the CPU (oracle layout [B][C][T]); the LeakyReLU branch is the kernel's own (the sign of its stored activation),
    # so that an activation within float32 noise of the kink cannot flip it
    y = Y.double().cpu().transpose(1, 2).contiguous().requires_grad_(True)
    gn = gain.double().cpu().view(1, C, 1).requires_grad_(True)
    bt = beta.double().cpu().view(1, C, 1).requires_grad_(True)
    xo = cln(y, gn, bt)
    pos = bf['out'][:, pad:].transpose(1, 2) > 0
    act = torch.where(pos, xo, SLOPE * xo)
    (act * dAct.double().cpu().transpose(1, 2)).sum().backward()
    n = C * torch.arange(1, T + 1, dtype=torch.float64)
    mu = y.detach().sum(1).cumsum(1) / n
    var = (y.detach().pow(2).sum(1).cumsum(1) - 2 * mu * y.detach().sum(1).cumsum(1)) / n + mu * mu
    r = 1 / (var + 1e-8).sqrt()
    what = 'T=%d C=%d' % (T, C)
    _check('nele_cln_fwd.mean', bf['mean'], mu, y.detach().abs().sum(1).cumsum(1) / n, c=1e-6, what=what)
    _check('nele_cln_fwd.rstd', bf['rstd'], r, r, c=1e-6, what=what)
    xh = (y.detach() - mu[:, None]) * r[:, None]
    S_out = ((y.detach().abs() + mu.abs()[:, None]) * r[:, None] * gn.detach().abs() + bt.detach().abs()).transpose(1, 2)
    _check('nele_cln_fwd.out', bf['out'][:, pad:], act.detach().transpose(1, 2), S_out, what=what)
    assert bool(torch.isnan(bf['out'][:, :pad]).all()), 'nele_cln_fwd wrote the rows before pad'
    # magnitudes of the backward's terms: dy = dx g r + RS_t + 2 y RQ_t with suffix sums RS, RQ over t' >= t
    dx = (dAct.double().cpu().transpose(1, 2) * torch.where(pos, 1.0, SLOPE)).detach()
    d = dx * gn.detach()
    A_abs, B_abs = d.abs().sum(1), (d * xh).abs().sum(1)
    ds_abs = (A_abs * r + B_abs * mu.abs() * r * r) / n
    dq_abs = B_abs * r * r / (2 * n)
    RS, RQ = ds_abs.flip(1).cumsum(1).flip(1), dq_abs.flip(1).cumsum(1).flip(1)
    S_dy = (d.abs() * r[:, None] + RS[:, None] + 2 * y.detach().abs() * RQ[:, None]).transpose(1, 2)
    ref_dy = y.grad.transpose(1, 2)
    _check('nele_cln_bwd.dY', bf['dY'][:, :T], ref_dy, S_dy, what=what)
    _check('nele_cln_bwd.dY16', bf['dY16'][:, :T], ref_dy, S_dy, bf16_out=True, what=what)
    assert bool(torch.isnan(bf['dY'][:, T:]).all() and torch.isnan(bf['dY16'][:, T:].float()).all()), 'nele_cln_bwd wrote the END padding'
    _check('nele_cln_bwd+colsum2.dgain', dg, gn.grad.view(C), (dx * xh).abs().sum((0, 2)), what=what)
    _check('nele_cln_bwd+colsum2.dbias', db, bt.grad.view(C), dx.abs().sum((0, 2)), what=what)


def test_cln_beyond_the_frame_limit_is_unsupported_and_writes_nothing():
    """T = 1025 > CLN_MAX_T: nele_cln_fwd and nele_cln_bwd return NELE_ERR_UNSUPPORTED and leave every output buffer as it was"""
    L = _lib()
    B, T, C, pad, pade = 1, 1025, 64, 4, 6
    Y = torch.randn((B, T, C), device='cuda')
    gain, beta = torch.ones(C, device='cuda'), torch.zeros(C, device='cuda')
    chunks = L.lib.nele_cln_chunks(T)
    bf = _cln_call_bufs(B, T, C, pad, pade, chunks)
    s = L.stream()
    assert L.lib.nele_cln_fwd(L.ptr(Y), L.ptr(gain), L.ptr(beta), L.ptr(bf['out']), L.ptr(bf['mean']), L.ptr(bf['rstd']), L.ptr(bf['scratch']), B, T, C, pad,
                              ctypes.c_float(SLOPE), s) == ERR_UNSUPPORTED
    bf['mean'].fill_(0.0)
    bf['rstd'].fill_(1.0)
    assert L.lib.nele_cln_bwd(L.ptr(Y), L.ptr(Y), L.ptr(gain), L.ptr(beta), L.ptr(bf['mean']), L.ptr(bf['rstd']), L.ptr(bf['dY']), L.ptr(bf['dY16']),
                              L.ptr(bf['gp']), L.ptr(bf['bp']), L.ptr(bf['scratch']), B, T, C, pade, ctypes.c_float(SLOPE), s) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    for k in ('out', 'dY', 'dY16', 'gp', 'bp'):
        assert bool(torch.isnan(bf[k].float()).all()), 'T=1025: %s was written' % k
    assert bool((bf['mean'] == 0).all() and (bf['rstd'] == 1).all())


# ------------------------------------------------------------------------------------------ 2. geometries the ABI accepts but the network does not use
def _c16_th(N, C, KH, KW, epi):
    """tile rows conv16 picks (c16_plan): a test-side mirror, used only to show that the sweep covers both"""
    TN, sps = (N + 15) // 16, (KW * C + 31) // 32
    if epi == EPI_MASK_LRELU_GRAD:
        return 4
    return 8 if KH * sps * TN <= 64 and TN <= 2 else 4


def _sweep():
    """seeded geometries: every TN class (N = 4 .. 64 in steps of 4), every channel / swizzle class (C = 8 .. 64), both tile heights,
    KH != KW, partial row / column tiles, output windows at nonzero offsets inside larger buffers"""
    rs = np.random.RandomState(20261016)
    Ns = [4, 12, 20, 40, 56, 64, 8, 16, 28, 32, 36, 44, 48, 52, 60, 24]
    Cs = [8, 16, 24, 32, 48, 64, 40, 56]
    out = []
    for i in range(36):
        N, C = Ns[i % len(Ns)], Cs[(i * 3) % len(Cs)]
        KH, KW = int(rs.randint(2, 10)), int(rs.randint(2, 10))
        if i % 4 == 0:
            KH, KW = 2 + i % 3, 3 + i % 5           # small kernels: the 8-row tiles of the forward pass
        B = 1 + i % 2
        Hout, Wout = int(rs.randint(1, 14)), int(rs.choice([1, 15, 16, 17, 63, 64, 65, 100, 130, 150]))
        eh, ew, ec = int(rs.randint(0, 4)), int(rs.randint(0, 5)), 4 * int(rs.randint(0, 3))
        out.append((B, N, C, KH, KW, Hout, Wout, eh, ew, ec, int(rs.randint(0, eh + 1)), int(rs.randint(0, ew + 1))))
    return out


SWEEP = _sweep()


def test_the_sweep_covers_every_class():
    tn = {(N + 15) // 16 for _, N, *_ in SWEEP}
    cs = {C for _, _, C, *_ in SWEEP}
    th = {_c16_th(N, C, KH, KW, EPI_BIAS_LRELU) for _, N, C, KH, KW, *_ in SWEEP}
    assert tn == {1, 2, 3, 4} and {8, 16, 24, 32, 48, 64} <= cs and th == {4, 8}
    assert {4, 12, 20, 40, 56} <= {N for _, N, *_ in SWEEP}
    assert sum(KH != KW for _, _, _, KH, KW, *_ in SWEEP) >= 20
    assert sum(oh0 > 0 or ow0 > 0 for *_, oh0, ow0 in SWEEP) >= 10


def _c16_window_case(L, B, N, C, KH, KW, Hout, Wout, OH, OW, OC, oh0, ow0, seed, out16, epi, expect_ok):
    H, W = Hout + KH - 1, Wout + KW - 1
    A, Wt, bias = _rand_conv(B, H, W, C, N, KH, KW, seed)
    geom = _geom(H, W, C, Hout, Wout, KH, KW, OH, OW, OC, 0, 0, oh0, ow0)
    M = B * Hout * Wout
    assert L.lib.nele_conv16_supported(M, N, geom, KH, KW) == int(expect_ok)
    wf = _frag16(L, _fwd_layout(Wt), N, C, KH, KW) if expect_ok else torch.zeros(64, dtype=torch.bfloat16, device='cuda')
    aux = torch.randn((B, Hout, Wout, N), device='cuda', generator=_gen(seed + 1)).to(torch.bfloat16)
    out = torch.full((B, OH, OW, OC), float('nan'), dtype=torch.bfloat16 if out16 else torch.float32, device='cuda')
    st = L.lib.nele_conv16(L.ptr(A), L.ptr(wf), L.ptr(bias), L.ptr(aux) if epi == EPI_MASK_LRELU_GRAD else None, L.ptr(out), out16, M, N, epi,
                           ctypes.c_float(SLOPE), geom, KH, KW, L.stream())
    torch.cuda.synchronize()
    if not expect_ok:
        assert st == ERR_UNSUPPORTED, st
        assert bool(torch.isnan(out.float()).all()), 'nele_conv16 declined the geometry but wrote its output'
        return
    assert st == 0, L.lib.nele_last_error_string()
    raw, S = _conv(A, Wt)
    if epi == EPI_MASK_LRELU_GRAD:
        m = torch.where(aux.double() > 0, 1.0, SLOPE)
        ref, S = raw * m, S * m
    else:
        ref, S = _lrelu(raw + bias.double()), S + bias.double().abs()
    win = out[:, oh0:oh0 + Hout, ow0:ow0 + Wout, :N]
    _check('nele_conv16.sweep', win, ref, S, bf16_out=bool(out16), what='B=%d N=%d C=%d %dx%d out %dx%d in %dx%dx%d at (%d, %d) epi=%d out16=%d' % (
        B, N, C, KH, KW, Hout, Wout, OH, OW, OC, oh0, ow0, epi, out16))
    inside = torch.zeros(out.shape, dtype=torch.bool, device='cuda')
    inside[:, oh0:oh0 + Hout, ow0:ow0 + Wout, :N] = True
    assert bool(torch.isnan(out[~inside].float()).all()), 'nele_conv16 wrote outside its output window (%d elements)' % int((~torch.isnan(out[~inside].float())).sum())


@pytest.mark.parametrize('case', range(len(SWEEP)))
def test_conv16_on_geometries_the_network_does_not_use(case):
    """nele_conv16 forward (bf16 and float32 stores) and mask gradient on a geometry nele_conv16_supported accepts: the output window at
    (oh0, ow0) of a larger OH x OW x OC buffer by the rule, every element outside the window still the NaN sentinel."""
    L = _lib()
    B, N, C, KH, KW, Hout, Wout, eh, ew, ec, oh0, ow0 = SWEEP[case]
    dims = (Hout, Wout, Hout + eh, Wout + ew, N + ec, oh0, ow0)
    for q, (epi, out16) in enumerate(((EPI_BIAS_LRELU, 1), (EPI_BIAS_LRELU, 0), (EPI_MASK_LRELU_GRAD, 1))):
        _c16_window_case(L, B, N, C, KH, KW, *dims, seed=1000 * case + q, out16=out16, epi=epi, expect_ok=True)


@pytest.mark.parametrize('N,C,KH,KW', [(68, 16, 3, 3), (16, 72, 3, 3), (16, 4, 3, 3), (16, 16, 1, 3), (16, 16, 3, 1), (16, 16, 3, 10), (6, 16, 3, 3),
                                       (16, 12, 3, 3)])
def test_conv16_declines_geometries_outside_its_contract(N, C, KH, KW):
    """where nele_conv16_supported returns 0, nele_conv16 returns NELE_ERR_UNSUPPORTED and leaves the output untouched"""
    _c16_window_case(_lib(), 1, N, C, KH, KW, 5, 20, 5, 20, N + (-N) % 4, 0, 0, seed=N * C + KH, out16=1, epi=EPI_BIAS_LRELU, expect_ok=False)


# ------------------------------------------------------------------------------------------ 3. the real discriminator plan, layer by layer
PREC_CODE = {'f32': 0, 'bf16': 1, 'bf16x3': 2}


def _ws_buffer(L, ws, B, T, prec, name):
    es = ctypes.c_int(0)
    p = L.lib.nele_disc_workspace_buffer(L.ptr(ws), B, T, 3, PREC_CODE[prec], name.encode(), ctypes.byref(es))
    return (p, es.value) if p else (None, 0)


def _ws_view(ws, ptr_, es, shape):
    off = ptr_ - ws.data_ptr()
    n = int(np.prod(shape))
    return ws[off:off + n * es].view(torch.bfloat16 if es == 2 else torch.float32).view(shape)


@pytest.mark.parametrize('prec,B,T,frames', [('bf16', 1, 52, None), ('bf16', 2, 53, None), ('bf16', 3, 149, None), ('bf16', 2, 40, None),
                                             ('bf16', 3, 149, (52, 97, 149)), ('f32', 2, 53, None), ('f32', 3, 149, (52, 97, 149)),
                                             ('bf16x3', 2, 53, None), ('bf16x3', 3, 149, (52, 97, 149))])
def test_discriminator_plan_layer_by_layer(prec, B, T, frames):
    """model.Discriminator forward + backward (need_din, weight gradients) on the library's plan; every layer's output checked against float64
    computed from the buffer the previous kernel actually stored, so that errors do not compound and the kernel-level rule applies: act[l]
    from act[l-1], pooled from act3, gbuf4 from the head's float64 gradient, gbuf[l-1] from gbuf[l] and act[l-1], ddin from gbuf0, and each
    conv layer's flat weight / bias gradient from conv2d_weight(act[l-1], gbuf[l]) through the spectral-norm chain rule
    (dW - <dW, W/sigma> u v^T) / sigma in float64.  Reference weights: bf16(float32(W_orig) * float32(1/sigma)) where the kernel takes bf16
    operands (weight_prep_kernel's arithmetic), the float32 product otherwise; f32 and bf16x3 run the same checks without operand rounding.
    Every gradient buffer's border is exactly zero.  The path is asserted: act1 is bf16 at T >= 52 in bf16, gbuf16 exists at T = 40."""
    from nele_gan_amd import model
    from weights_recipe import seeded_state_arrays
    import capi_nets as cn
    L = _lib()
    D = model.Discriminator(nout=3)
    st = seeded_state_arrays(cn.d_keys_shapes(3, 3), 202 + T)
    D.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    D = D.cuda()
    D.precision = prec
    D.train()
    g = _gen(31 * T + B)
    din = torch.zeros((B, 64, T, 4), device='cuda')
    din[..., :3] = torch.rand((B, 64, T, 3), device='cuda', generator=g)
    fr = None
    if frames is not None:
        fr = torch.tensor(frames, dtype=torch.int32, device='cuda')
        for b, f in enumerate(frames):
            din[b, :, f:] = 0
    dsc = torch.randn((B, 3), device='cuda', generator=g)
    D.flat_parameters().grad.zero_()
    x = din.clone().requires_grad_(True)
    score = D.forward_packed(x, fr)
    (score * dsc).sum().backward()
    torch.cuda.synchronize()
    (ws,) = [w.buf for w in D._bufs.values()]
    bufs = {}
    dims = _d_dims(T)
    for name in ['act%d' % l for l in range(5)] + ['gbuf%d' % l for l in range(5)] + ['gbuf16', 'pooled', 'ddin', 'sigma']:
        bufs[name] = _ws_buffer(L, ws, B, T, prec, name)
    assert bufs['sigma'][0] is not None and bufs['sigma'][1] == 4
    sigma = _ws_view(ws, bufs['sigma'][0], 4, (8,)).double()
    c16 = bufs['act1'][1] == 2
    if prec == 'bf16':
        assert c16 == (T >= 52), 'bf16: act1 element size %d at T = %d' % (bufs['act1'][1], T)
        # the bf16 pooling gradient exists where conv16 is not used and the span / tile kernels take D.conv5's data / weight gradients
        (Hi4, Wi4, Ci4), (Ho4, Wo4, _) = dims[4], dims[5]
        g4b = _geom(Ho4 + 16, Wo4 + 16, 64, Hi4, Wi4, 9, 9, Hi4 + 12, Wi4 + 12, Ci4, 0, 0, 6, 6)
        g4w = _geom(Hi4, Wi4, Ci4, Ho4, Wo4, 9, 9, Ho4 + 16, Wo4 + 16, 64, 0, 0, 8, 8)
        want16 = not c16 and L.lib.nele_conv_span_bf16_a16_supported(B * Hi4 * Wi4, Ci4, g4b, 9, 9) == 1 and \
            L.lib.nele_conv_wgrad_bf16_d16_supported(B * Ho4 * Wo4, 64, g4w, 9, 9) == 1
        assert (bufs['gbuf16'][0] is not None) == want16, 'bf16: gbuf16 at T = %d' % T
    else:
        assert not c16 and bufs['gbuf16'][0] is None
    wv = [T - 20] * B if frames is None else [f - 20 for f in frames]
    act = [_ws_view(ws, bufs['act%d' % l][0], bufs['act%d' % l][1], (B,) + dims[l + 1]) for l in range(5)]
    pads = [k - 1 for _, k in D_CONVS]
    gbuf = [_ws_view(ws, bufs['gbuf%d' % l][0], bufs['gbuf%d' % l][1], (B, dims[l + 1][0] + 2 * pads[l], dims[l + 1][1] + 2 * pads[l], dims[l + 1][2]))
            for l in range(5)]
    glast = gbuf[4] if bufs['gbuf16'][0] is None else _ws_view(ws, bufs['gbuf16'][0], 2, gbuf[4].shape)
    b16 = prec == 'bf16'

    def rounded(fn, M, N, geom, k):            # does this pass take bf16 operands? (conv16 always; the span kernel where it takes the geometry)
        return b16 and (c16 or L.lib.nele_conv_span_bf16_supported(M, N, geom, k, k) == 1)

    def weight(l, rnd):
        Wo_ = getattr(D.layers[l], 'weight_orig').detach().float()
        w = Wo_ * (1.0 / sigma[l].float())
        return (_r16(w) if rnd else w).double()

    tag = '%s B=%d T=%d frames=%s' % (prec, B, T, frames)
    # ---- forward
    xin = din[..., :3]
    for l in range(5):
        (Hi, Wi, Ci), (Ho, Wo, co), k = dims[l], dims[l + 1], D_CONVS[l][1]
        a_prev = xin if l == 0 else act[l - 1]
        geom = _geom(Hi, Wi, Ci, Ho, Wo, k, k, Ho, Wo, co)
        rnd = (l > 0 or not c16) and rounded('f', B * Ho * Wo, co, geom, k)      # (D.layers.0 in bf16 is float32-exact on conv16's path)
        a_op = a_prev.double() if not rnd else _r16(a_prev.float()).double()
        bias = D.layers[l].bias.detach().double()
        raw, S = _conv(a_op, weight(l, rnd))
        ref, S = _lrelu(raw + bias), S + bias.abs()
        if l == 0 and c16:                     # nele_conv16_pointwise_fwd: float32-exact, stored as bf16
            steps = (act[0].view(torch.int16).int() - ref.to(torch.bfloat16).view(torch.int16).int()).abs()
            assert int(steps.max()) <= 1, '%s act0: %d bf16 steps' % (tag, int(steps.max()))
        else:
            _check('plan.%s.act%d' % (prec, l), act[l], ref, S, bf16_out=act[l].dtype == torch.bfloat16, what=tag)
        if l == 4:
            pooled = _ws_view(ws, bufs['pooled'][0], 4, (B, 64))
            rp = torch.stack([ref[b, :, :wv[b]].mean((0, 1)) for b in range(B)])
            sp = torch.stack([S[b, :, :wv[b]].mean((0, 1)) for b in range(B)])
            _check('plan.%s.pooled' % prec, pooled, rp, sp, what=tag)
    # ---- the head's gradient into the pooling gradient buffer, from the kernel's pooled
    hw = [(getattr(D, n).weight_orig.detach(), getattr(D, n).bias.detach()) for n in ('fc1', 'fc2', 'fc3')]
    pl = pooled.double().clone().requires_grad_(True)
    z, s_mag, zs = pl, pl.detach().abs(), []
    for q, (w, bb) in enumerate(hw):
        wn = w.double() / sigma[5 + q]
        z = z @ wn.T + bb.double()
        zs.append(z)
        s_mag = s_mag @ wn.abs().T + bb.double().abs()
        z = _lrelu(z) if q < 2 else torch.sigmoid(z)
    _check('plan.%s.score' % prec, score.detach(), z.detach(), s_mag, what=tag)
    (z * dsc.double()).sum().backward()
    s = (dsc.double() * z.detach() * (1 - z.detach())).abs()
    for q in (2, 1, 0):
        s = s @ (hw[q][0].double() / sigma[5 + q]).abs()
        if q > 0:
            s = s * torch.where(zs[q - 1].detach() > 0, 1.0, SLOPE)
    Ho, Wo = dims[5][0], dims[5][1]
    m4 = torch.where(act[4].double() > 0, 1.0, SLOPE)
    inner = glast[:, 8:8 + Ho, 8:8 + Wo].double()
    for b in range(B):
        n = Ho * wv[b]
        _check('plan.%s.gbuf4' % prec, inner[b, :, :wv[b]], pl.grad[b] / n * m4[b, :, :wv[b]], s[b] / n * m4[b, :, :wv[b]],
               bf16_out=glast.dtype == torch.bfloat16, what=tag)
        assert bool((inner[b, :, wv[b]:] == 0).all()), '%s: pooling gradient beyond wvalid' % tag
    _border_is_zero(glast, 8, 'plan gbuf4 ' + tag)
    # ---- data gradients: gbuf[l-1] from gbuf[l] (glast for l = 4) and act[l-1]; ddin from gbuf0
    for l in (4, 3, 2, 1, 0):
        (Hi, Wi, Ci), (Ho, Wo, co), k = dims[l], dims[l + 1], D_CONVS[l][1]
        p = k - 1
        src = glast if l == 4 else gbuf[l]
        pp = pads[l - 1] if l > 0 else 0
        geom = _geom(Ho + 2 * p, Wo + 2 * p, co, Hi, Wi, k, k, Hi + 2 * pp, Wi + 2 * pp, Ci, 0, 0, pp, pp)
        rnd = l > 0 and rounded('b', B * Hi * Wi, Ci, geom, k)
        src_op = _r16(src.float()).double() if rnd else src.double()
        Wl = weight(l, rnd)
        if l == 0:
            Wl = torch.cat([Wl, torch.zeros_like(Wl[:, :1])], 1)            # ddin's 4th (zero) channel
        raw, S = _conv(src_op, _flip_weight(Wl))
        if l > 0:
            m = torch.where(act[l - 1].double() > 0, 1.0, SLOPE)
            out = gbuf[l - 1]
            _check('plan.%s.gbuf%d' % (prec, l - 1), out[:, pp:pp + Hi, pp:pp + Wi], raw * m, S * m, bf16_out=out.dtype == torch.bfloat16, what=tag)
            _border_is_zero(out, pp, 'plan gbuf%d %s' % (l - 1, tag))
        else:
            ddin = _ws_view(ws, bufs['ddin'][0], 4, (B, 64, T, 4))
            _check('plan.%s.ddin' % prec, ddin, raw, S, what=tag)
    # ---- weight and bias gradients through the spectral-norm chain rule
    for l in range(5):
        (Hi, Wi, Ci), (Ho, Wo, co), k = dims[l], dims[l + 1], D_CONVS[l][1]
        p = k - 1
        dsrc = (glast if l == 4 else gbuf[l])[:, p:p + Ho, p:p + Wo]
        a_prev = xin if l == 0 else act[l - 1]
        rnd = b16 and l > 0                    # every bf16 weight-gradient entry point rounds its operands
        a_op = _r16(a_prev.float()) if rnd else a_prev.float()
        d_op = _r16(dsrc.float()) if rnd else dsrc.float()
        cv = 3 if l == 0 else Ci
        G, SG = _wgrad_ref(a_op, d_op, (co, cv, k, k))
        W = D.layers[l].weight_orig.detach().double()
        u, v = D.layers[l].weight_u.detach().double(), D.layers[l].weight_v.detach().double()
        sg = sigma[l]
        uv = torch.outer(u, v).view_as(W)
        ref = (G - (G * W / sg).sum() * uv) / sg
        S = (SG + (SG * W.abs() / sg).sum() * uv.abs()) / sg
        _check('plan.%s.dW%d' % (prec, l), D.layers[l].weight_orig.grad, ref, S, what=tag)
        rb, sb = dsrc.double().sum((0, 1, 2)), dsrc.double().abs().sum((0, 1, 2))
        rb16 = d_op.double().sum((0, 1, 2))
        got_b = D.layers[l].bias.grad.double()
        ok_b = ((got_b - rb).abs() <= C32 * sb) | ((got_b - rb16).abs() <= C32 * sb)
        assert bool(ok_b.all()), '%s db%d' % (tag, l)
