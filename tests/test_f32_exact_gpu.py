"""GPU: the float32 dense kernels of dense.hip on their own, against float64 on the float32 values they read.

nele_conv_gemm (all twelve conv_gemm_kernel<TN, TM>), nele_conv_span + nele_weight_prep_frag (conv_span_kernel<1..4>), nele_conv_wgrad
in float32 (conv_wgrad_kernel, conv_wgrad_pointwise_kernel, wgrad_reduce_kernel), nele_weight_prep and nele_weight_prep_batch.  Two rules
(tests/exact_rules.py, tests/f32_cases.py):

  1. random operands (normal, weights / sqrt(K)):  |got - ref| <= 2e-5 S,  S = sum |a w| per output element.  One missing tap at K = 3888
     is off by about 1 / 3888 = 2.6e-4 S.
  2. integer operands (activations in {-4..4}, weights and gradients in {-2..2}): every partial sum is an integer below 2^24, so any
     summation order is exact and the output must EQUAL the float64 result, bit for bit.  The precondition is asserted from S.

Output buffers start as NaN; the input window sits inside a NaN buffer too, so that a read outside it poisons the result.  What the
contract does not write must still be NaN.  The shapes are the smallest that reach each code path; see f32_cases.py for why each is there.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import f32_cases as cases  # noqa: E402
from exact_rules import (C32, EPI_BIAS, EPI_BIAS_EXPTANH, EPI_BIAS_LRELU, EPI_MASK_LRELU_GRAD, EPI_NONE, ERR_UNSUPPORTED, ERR_WORKSPACE,  # noqa: E402,F401
                         MARGINS, P_, SLOPE, _check, _conv, _flip_layout, _flip_weight, _fwd_layout, _gen, _geom, _lib, _report_margins,
                         _wgrad_ref)
from test_bf16x3_gpu import EXPTANH_ERR  # noqa: E402  (the derived bound of the exp(3.2 tanh) store epilogue)

NAN = float('nan')


def _ints(shape, hi, g):
    return torch.randint(-hi, hi + 1, shape, device='cuda', generator=g).float()


def _operands(a_shape, w_shape, K, ints, seed):
    """activation and weight of one rule: integer {-4..4} / {-2..2}, or normal with the weight scaled by 1 / sqrt(K)"""
    g = _gen(seed)
    if ints:
        return _ints(a_shape, cases.INT_A, g), _ints(w_shape, cases.INT_W, g)
    return torch.randn(a_shape, device='cuda', generator=g), torch.randn(w_shape, device='cuda', generator=g) / np.sqrt(K)


def _window_call(L, kind, win, Wg, N, KH, KW, epi=EPI_NONE, bias=None, aux_seed=None, offs=(1, 2, 2, 1), oc_extra=4):
    """nele_conv_gemm ('gemm') or nele_weight_prep_frag + nele_conv_span ('span') on the window `win` [B][H][W][C], placed at (ih0, iw0) of a NaN
    buffer, writing the valid convolution at (oh0, ow0) of a NaN buffer [B][Hout + oh0 + 1][Wout + ow0 + 2][N + oc_extra].
    -> (status, out buffer, the window of the output, aux or None)"""
    ih0, iw0, oh0, ow0 = offs
    B, H, W, C = win.shape
    Hout, Wout = H - KH + 1, W - KW + 1
    A = torch.full((B, H + ih0 + 1, W + iw0 + 2, C), NAN, device='cuda')
    A[:, ih0:ih0 + H, iw0:iw0 + W] = win
    OH, OW, OC = Hout + oh0 + 1, Wout + ow0 + 2, N + oc_extra
    out = torch.full((B, OH, OW, OC), NAN, device='cuda')
    geom = _geom(A.shape[1], A.shape[2], C, Hout, Wout, KH, KW, OH, OW, OC, ih0, iw0, oh0, ow0)
    M = B * Hout * Wout
    aux = None
    if aux_seed is not None:
        aux = torch.randn((B, Hout, Wout, OC), device='cuda', generator=_gen(aux_seed))
    if kind == 'gemm':
        st = L.lib.nele_conv_gemm(L.ptr(A), L.ptr(Wg), L.ptr(bias), L.ptr(aux), L.ptr(out), M, N, epi, SLOPE, geom, L.stream())
    else:
        Ktot = KH * KW * C
        frag = torch.full((max(Ktot // 8, 1) * ((N + 15) // 16) * 128,), NAN, device='cuda')
        if L.lib.nele_conv_span_supported(M, N, geom, KH, KW) == 1:
            L.call('nele_weight_prep_frag', L.ptr(Wg), N, Ktot, L.ptr(frag), L.stream())
        st = L.lib.nele_conv_span(L.ptr(A), L.ptr(frag), L.ptr(bias), L.ptr(aux), L.ptr(out), M, N, epi, SLOPE, geom, KH, KW, A.numel(), L.stream())
    torch.cuda.synchronize()
    return st, out, out[:, oh0:oh0 + Hout, ow0:ow0 + Wout, :N], aux


def _untouched_outside(out, offs, Hout, Wout, N, what):
    oh0, ow0 = offs[2], offs[3]
    inside = torch.zeros(out.shape, dtype=torch.bool, device='cuda')
    inside[:, oh0:oh0 + Hout, ow0:ow0 + Wout, :N] = True
    assert bool(torch.isnan(out[~inside]).all()), '%s wrote outside its output window (%d elements)' % (what, int((~torch.isnan(out[~inside])).sum()))


def _conv_inputs(B, Hout, Wout, C, N, KH, KW, dgrad, ints, seed):
    """-> window [B][H][W][C], GEMM-layout weight [N][KH KW C], the equivalent forward weight [N][C][KH][KW] of the float64 reference.
    dgrad: the window is the output gradient of a C <- N layer inside a zero border of (KH - 1, KW - 1) (less where the window is too small
    to hold one: at least one row and column of gradient stay), the weight that layer's, flipped"""
    K = KH * KW * C
    H, W = Hout + KH - 1, Wout + KW - 1
    if not dgrad:
        win, Wt = _operands((B, H, W, C), (N, C, KH, KW), K, ints, seed)
        return win, _fwd_layout(Wt), Wt
    win, Wt = _operands((B, H, W, C), (C, N, KH, KW), K, ints, seed)                               # the layer: N inputs -> C outputs
    bh, bw = min(KH - 1, (H - 1) // 2), min(KW - 1, (W - 1) // 2)
    keep = torch.zeros((H, W), dtype=torch.bool, device='cuda')
    keep[bh:H - bh, bw:W - bw] = True
    win = win * keep[None, :, :, None]
    return win, _flip_layout(Wt), _flip_weight(Wt)


def _both_rules(L, kind, name, tag, B, Hout, Wout, C, N, KH, KW, dgrad, seed, offs=(1, 2, 2, 1)):
    """the two rules of the module docstring on one geometry; -> the integer-rule output window (for span == gemm)"""
    for ints in (False, True):
        win, Wg, Wt = _conv_inputs(B, Hout, Wout, C, N, KH, KW, dgrad, ints, seed + int(ints))
        st, out, got, _ = _window_call(L, kind, win, Wg, N, KH, KW, offs=offs)
        assert st == 0, '%s %s: status %d %s' % (name, tag, st, L.lib.nele_last_error_string())
        ref, S = _conv(win, Wt)
        what = '%s ints=%d' % (tag, ints)
        if ints:
            assert float(S.max()) < cases.LIMIT, '%s: the integer rule needs every |sum| < 2^24 (S = %g)' % (what, float(S.max()))
            bad = got != ref.float()
            assert not bool(bad.any()), '%s %s: %d of %d elements differ from the exact result; first at %s' % (
                name, what, int(bad.sum()), bad.numel(), tuple(int(i) for i in bad.nonzero()[0]))
        else:
            _check(name, got, ref, S, what=what)
        _untouched_outside(out, offs, Hout, Wout, N, name + ' ' + what)
    return got


# ------------------------------------------------------------------------------------------ nele_conv_gemm
GEMM_CASES = cases.gemm_cases()


@pytest.mark.parametrize('case', GEMM_CASES, ids=[c[0] for c in GEMM_CASES])
def test_conv_gemm_forward_and_data_gradient(case):
    """nele_conv_gemm at every TN, at G's and D's own geometries (forward, and the data-gradient form: flipped weights over the zero-bordered
    gradient) and at a K that is no multiple of the K step, with the input window at (ih0, iw0) = (1, 2) and the output window at
    (oh0, ow0) = (2, 1) of larger buffers: both rules; everything outside the output window still NaN."""
    L = _lib()
    tag, B, Hout, Wout, C, N, KH, KW, dgrad = case
    _both_rules(L, 'gemm', 'nele_conv_gemm' + ('.dgrad' if dgrad else ''), tag, B, Hout, Wout, C, N, KH, KW, dgrad, 7000 + 13 * GEMM_CASES.index(case))


TM_CASES = cases.gemm_tm_cases()


@pytest.mark.parametrize('N,M,tm', TM_CASES)
def test_conv_gemm_rows_per_block_variants(N, M, tm):
    """every TM of every TN: Linear-shaped problems (KH = KW = 1, C = 16) with M on both sides of the thresholds of the host's chip-fill
    rule (derived in f32_cases.py), each with a partial last block.  Both rules."""
    L = _lib()
    assert cases.gemm_tm(M, N) == tm
    _both_rules(L, 'gemm', 'nele_conv_gemm.TM%d' % tm, 'N=%d M=%d' % (N, M), 1, 1, M, 16, N, 1, 1, False, 8000 + N + M, offs=(0, 3, 0, 2))


@pytest.mark.parametrize('kind,N,C,KH,KW,Wout', [('gemm', 20, 8, 3, 3, 37), ('gemm', 80, 8, 3, 3, 37), ('span', 48, 32, 3, 3, 67)])
def test_store_epilogues_equal_the_plain_output_post_processed(kind, N, C, KH, KW, Wout):
    """EPI_BIAS, EPI_BIAS_LRELU and EPI_MASK_LRELU_GRAD are one float32 add and one select or multiply on the EPI_NONE output: bit for bit;
    EPI_BIAS_EXPTANH within the float32 rounding of its steps (EXPTANH_ERR, derived in test_bf16x3_gpu.py).  aux is read as [M][OC]."""
    L = _lib()
    B, Hout = 2, 5
    win, Wg, _ = _conv_inputs(B, Hout, Wout, C, N, KH, KW, False, False, 4242 + N)
    bias = torch.randn(N, device='cuda', generator=_gen(4243))
    sl = torch.tensor(SLOPE, dtype=torch.float32, device='cuda')
    st, _, plain, _ = _window_call(L, kind, win, Wg, N, KH, KW)
    assert st == 0 and not bool(torch.isnan(plain).any())
    vb = plain + bias
    for epi, want in ((EPI_BIAS, vb), (EPI_BIAS_LRELU, torch.where(vb > 0, vb, sl * vb))):
        st, out, got, _ = _window_call(L, kind, win, Wg, N, KH, KW, epi=epi, bias=bias)
        assert st == 0 and torch.equal(got, want), (kind, epi)
        _untouched_outside(out, (1, 2, 2, 1), Hout, Wout, N, '%s epi %d' % (kind, epi))
    st, out, got, aux = _window_call(L, kind, win, Wg, N, KH, KW, epi=EPI_MASK_LRELU_GRAD, aux_seed=99)
    assert st == 0 and torch.equal(got, torch.where(aux[..., :N] > 0, plain, sl * plain))
    st, out, got, _ = _window_call(L, kind, win, Wg, N, KH, KW, epi=EPI_BIAS_EXPTANH, bias=bias)
    ref = torch.exp(3.2 * torch.tanh(plain.double() + bias.double()))
    err = float(((got.double() - ref).abs() / ref).max())
    print('exptanh relative error', kind, N, err)
    assert st == 0 and err <= EXPTANH_ERR, (kind, err)


# ------------------------------------------------------------------------------------------ nele_conv_span
@pytest.mark.parametrize('Wout', cases.SPAN_WIDTHS)
def test_conv_span_at_the_discriminator_layers(Wout):
    """nele_weight_prep_frag + nele_conv_span at D.layers.1-4 forward, their data gradients and the 8 -> 4 pointwise data gradient (NT = 1..4,
    N = 4 .. 64), B = 3 with 3 or 4 output rows: a block's runs straddle rows and utterances.  nele_conv_span_supported is 1 for every case
    (worked out by hand in f32_cases.py).  Both rules, and under the integer rule nele_conv_gemm on the same inputs gives the same bits."""
    L = _lib()
    Hout, ran = cases.span_hout(Wout), 0
    for q, (tag, C, N, K) in enumerate(cases.SPAN_LAYERS):
        dgrad = tag.endswith('dgrad')
        args = (cases.SPAN_B, Hout, Wout, C, N, K, K, dgrad, 9000 + 100 * q + Wout)
        geom = _geom(Hout + K + 1, Wout + K + 3, C, Hout, Wout, K, K, Hout + 3, Wout + 3, N + 4, 1, 2, 2, 1)
        assert L.lib.nele_conv_span_supported(cases.SPAN_B * Hout * Wout, N, geom, K, K) == 1, (tag, Wout)
        span = _both_rules(L, 'span', 'nele_conv_span' + ('.dgrad' if dgrad else ''), '%s Wout=%d' % (tag, Wout), *args)
        win, Wg, _ = _conv_inputs(*args[:-1], True, args[-1] + 1)          # the integer-rule inputs of _both_rules
        st, _, gemm, _ = _window_call(L, 'gemm', win, Wg, N, K, K)
        assert st == 0 and torch.equal(span, gemm), 'span != gemm on integer operands: %s Wout=%d' % (tag, Wout)
        ran += 1
    assert ran == 9


@pytest.mark.parametrize('what,N,C,K,Wout', [('N=80', 80, 8, 3, 70), ('Wout=63', 16, 8, 3, 63), ('seglen=12', 16, 4, 3, 70)])
def test_conv_span_declines_geometries_outside_its_contract(what, N, C, K, Wout):
    """where nele_conv_span_supported returns 0, nele_conv_span returns NELE_ERR_UNSUPPORTED and leaves the output untouched"""
    L = _lib()
    win, Wg, _ = _conv_inputs(2, 3, Wout, C, N, K, K, False, False, 77)
    geom = _geom(3 + K + 1, Wout + K + 3, C, 3, Wout, K, K, 6, Wout + 3, N + 4, 1, 2, 2, 1)
    assert L.lib.nele_conv_span_supported(2 * 3 * Wout, N, geom, K, K) == 0
    st, out, _, _ = _window_call(L, 'span', win, Wg, N, K, K)
    assert st == ERR_UNSUPPORTED, st
    assert bool(torch.isnan(out).all()), 'nele_conv_span declined %s but wrote its output' % what


# ------------------------------------------------------------------------------------------ nele_conv_wgrad (float32)
WGRAD_CASES = cases.wgrad_cases()


def _wgrad_buffers(B, Hout, Wout, C, N, KH, KW, pad, ints, seed):
    """-> A [B][H][W][C], the output-gradient buffer, its region of the output positions, geom.  pad: zero border of the gradient buffer on
    every side (D's gbuf), None: KW - 1 columns of END padding (G's dY)"""
    g = _gen(seed)
    H, W = Hout + KH - 1, Wout + KW - 1
    if ints:
        A, dOin = _ints((B, H, W, C), cases.INT_A, g), _ints((B, Hout, Wout, N), cases.INT_W, g)
    else:
        A, dOin = torch.randn((B, H, W, C), device='cuda', generator=g), 0.1 * torch.randn((B, Hout, Wout, N), device='cuda', generator=g)
    if pad is None:
        dO = torch.zeros((B, Hout, Wout + KW - 1, N), device='cuda')
        dO[:, :, :Wout] = dOin
        geom = _geom(H, W, C, Hout, Wout, KH, KW, Hout, Wout + KW - 1, N)
    else:
        dO = torch.zeros((B, Hout + 2 * pad, Wout + 2 * pad, N), device='cuda')
        dO[:, pad:pad + Hout, pad:pad + Wout] = dOin
        geom = _geom(H, W, C, Hout, Wout, KH, KW, Hout + 2 * pad, Wout + 2 * pad, N, 0, 0, pad, pad)
    return A, dO, dOin, geom


@pytest.mark.parametrize('case', WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_conv_wgrad_f32(case):
    """nele_conv_wgrad, dW and db, at D.layers.1-4 and G's layers (one split at M = 80, many elsewhere), with a last split of one and of three
    rows, and on the pointwise kernel with 3 valid channels of 4 (dW [N][3][1][1]) at 1, 5 and the capped 64 splits; accumulate = 0 into NaN
    and accumulate = 1 onto known values (random rule: one float32 rounding of the sum allowed; integer rule: integers, still exact).
    Nothing is written behind dW or db."""
    L = _lib()
    tag, B, Hout, Wout, C, Cv, N, KH, KW, pad = case
    M, Ktot = B * Hout * Wout, KH * KW * C
    splits = ctypes.c_int(0)
    nws = int(L.lib.nele_conv_wgrad_workspace_floats(M, N, Ktot, ctypes.byref(splits)))
    if tag.startswith('last-split'):
        assert splits.value == 17 and M - 16 * 512 in (1, 3)
    if tag.startswith('G') and 'T40' in tag:
        assert splits.value == 1
    nW = N * Cv * KH * KW
    for ints in (False, True):
        A, dO, dOin, geom = _wgrad_buffers(B, Hout, Wout, C, N, KH, KW, pad, ints, 5000 + 2 * WGRAD_CASES.index(case) + int(ints))
        if Cv < C:
            A[..., Cv:] = 1e4 if not ints else 4.0            # channels >= Cvalid must not leak in
        rW, sW = _wgrad_ref(A[..., :Cv], dOin, (N, Cv, KH, KW))
        rb, sb = dOin.double().sum((0, 1, 2)), dOin.double().abs().sum((0, 1, 2))
        if ints:
            assert float(sW.max()) + cases.INT_A * cases.INT_W < cases.LIMIT and float(sb.max()) + cases.INT_W < cases.LIMIT
        for acc in (0, 1):
            g = _gen(31 + acc)
            dW, db = torch.full((nW + 64,), NAN, device='cuda'), torch.full((N + 4,), NAN, device='cuda')
            bw = bb = None
            if acc:
                bw = _ints((nW,), 8, g) if ints else torch.randn(nW, device='cuda', generator=g)
                bb = _ints((N,), 2, g) if ints else torch.randn(N, device='cuda', generator=g)
                dW[:nW], db[:N] = bw, bb
            wsb = torch.full((nws,), NAN, device='cuda')
            L.call('nele_conv_wgrad', L.ptr(A), L.ptr(dO), L.ptr(wsb), nws, M, N, geom, KH, KW, Cv, L.ptr(dW), L.ptr(db), acc, L.stream())
            torch.cuda.synchronize()
            what = '%s ints=%d accumulate=%d' % (tag, ints, acc)
            wantW = rW + (bw.double().view_as(rW) if acc else 0)
            wantb = rb + (bb.double() if acc else 0)
            gotW = dW[:nW].view(N, Cv, KH, KW)
            if ints:
                assert torch.equal(gotW, wantW.float()), 'nele_conv_wgrad %s: %d dW elements differ from the exact result' % (what, int((gotW != wantW.float()).sum()))
                assert torch.equal(db[:N], wantb.float()), 'nele_conv_wgrad %s: db differs from the exact result' % what
            else:
                ulp = 2 ** -23 / C32                          # accumulate: one float32 rounding of old + new
                _check('nele_conv_wgrad', gotW, wantW, sW + (ulp * bw.abs().view_as(rW) if acc else 0), what=what)
                _check('nele_conv_wgrad.db', db[:N], wantb, sb + (ulp * bb.abs() if acc else 0), what=what)
            assert bool(torch.isnan(dW[nW:]).all() and torch.isnan(db[N:]).all()), 'nele_conv_wgrad %s: wrote past dW / db' % what


def test_conv_wgrad_with_a_workspace_too_small_writes_nothing():
    """one float short of nele_conv_wgrad_workspace_floats: NELE_ERR_WORKSPACE, and dW, db and the workspace stay as they were"""
    L = _lib()
    B, Hout, Wout, C, N, K = 2, 20, 30, 8, 16, 3
    A, dO, _, geom = _wgrad_buffers(B, Hout, Wout, C, N, K, K, 2, False, 1)
    M = B * Hout * Wout
    nws = int(L.lib.nele_conv_wgrad_workspace_floats(M, N, K * K * C, None))
    dW, db, wsb = torch.full((N * C * K * K,), NAN, device='cuda'), torch.full((N,), NAN, device='cuda'), torch.full((nws,), NAN, device='cuda')
    st = L.lib.nele_conv_wgrad(L.ptr(A), L.ptr(dO), L.ptr(wsb), nws - 1, M, N, geom, K, K, C, L.ptr(dW), L.ptr(db), 0, L.stream())
    torch.cuda.synchronize()
    assert st == ERR_WORKSPACE, st
    assert bool(torch.isnan(dW).all() and torch.isnan(db).all() and torch.isnan(wsb).all())


# ------------------------------------------------------------------------------------------ nele_weight_prep, nele_weight_prep_batch
PREP_SHAPES = [(16, 8, 8, 3, 3), (8, 3, 4, 1, 1), (64, 48, 48, 9, 9), (256, 128, 128, 1, 5), (12, 5, 8, 2, 3)]   # (N, Cvalid, C, KH, KW)


def _prep_ref(Wt, sigma, C):
    """float32 torch: Wt * (1 / sigma) permuted to Wf [N][KH][KW][C] (channels >= Cvalid left out) and flipped to Wb [Cvalid][KH][KW][N]"""
    v = Wt * (1.0 / sigma[0]) if sigma is not None else Wt
    return v.permute(0, 2, 3, 1).contiguous(), v.flip(2, 3).permute(1, 2, 3, 0).contiguous()


@pytest.mark.parametrize('N,Cv,C,KH,KW', PREP_SHAPES)
def test_weight_prep_is_a_permute_and_flip_of_the_scaled_weight(N, Cv, C, KH, KW):
    """Wf and Wb bit-equal to a torch permute / flip of Wt * (1 / sigma) in float32 (and of Wt itself without sigma); with Cvalid < C the kernel
    writes only ci < Cvalid: zero-filled padding stays zero, NaN-filled padding stays NaN - zeroing it is the caller's job."""
    L = _lib()
    g = _gen(N + C)
    Wt = torch.randn((N, Cv, KH, KW), device='cuda', generator=g)
    for sigma in (torch.tensor([1.7], device='cuda'), None):
        wf_ref, wb_ref = _prep_ref(Wt, sigma, C)
        for fill in (0.0, NAN):
            Wf = torch.full((N, KH, KW, C), fill, device='cuda')
            Wb = torch.full((Cv * KH * KW * N + 16,), NAN, device='cuda')
            L.call('nele_weight_prep', L.ptr(Wt), L.ptr(sigma), N, Cv, C, KH, KW, L.ptr(Wf), L.ptr(Wb), L.stream())
            torch.cuda.synchronize()
            assert torch.equal(Wf[..., :Cv], wf_ref)
            assert torch.equal(Wb[:-16].view(Cv, KH, KW, N), wb_ref) and bool(torch.isnan(Wb[-16:]).all())
            pad = Wf[..., Cv:]
            assert bool((pad == 0).all() if fill == 0.0 else torch.isnan(pad).all()), 'nele_weight_prep wrote the padded channels'
        Wf = torch.full((N, KH, KW, C), 0.0, device='cuda')
        L.call('nele_weight_prep', L.ptr(Wt), L.ptr(sigma), N, Cv, C, KH, KW, L.ptr(Wf), None, L.stream())     # Wb = NULL
        torch.cuda.synchronize()
        assert torch.equal(Wf[..., :Cv], wf_ref)


def test_weight_prep_batch_equals_the_single_form():
    """two jobs of different shape (one with sigma and Wb, one without either) in one launch: bit-equal to nele_weight_prep per job"""
    L = _lib()
    g = _gen(5)
    jobs = [(PREP_SHAPES[0], torch.tensor([0.8], device='cuda'), True), (PREP_SHAPES[4], None, False), (PREP_SHAPES[1], torch.tensor([2.5], device='cuda'), True)]
    ptrs, dims, outs = [], [], []
    for (N, Cv, C, KH, KW), sigma, wb in jobs:
        Wt = torch.randn((N, Cv, KH, KW), device='cuda', generator=g)
        Wf1, Wf2 = (torch.full((N, KH, KW, C), NAN, device='cuda') for _ in range(2))
        Wb1, Wb2 = ((torch.full((Cv, KH, KW, N), NAN, device='cuda') if wb else None) for _ in range(2))
        L.call('nele_weight_prep', L.ptr(Wt), L.ptr(sigma), N, Cv, C, KH, KW, L.ptr(Wf1), L.ptr(Wb1), L.stream())
        ptrs += [Wt.data_ptr(), sigma.data_ptr() if sigma is not None else None, Wf2.data_ptr(), Wb2.data_ptr() if wb else None]
        dims += [N, Cv, C, KH, KW]
        outs.append((Wt, sigma, Wf1, Wf2, Wb1, Wb2))
    L.call('nele_weight_prep_batch', (P_ * len(ptrs))(*ptrs), (ctypes.c_int * len(dims))(*dims), len(jobs), L.stream())
    torch.cuda.synchronize()
    for (shape, _, wb), (Wt, sigma, Wf1, Wf2, Wb1, Wb2) in zip(jobs, outs):
        Cv = shape[1]
        assert torch.equal(Wf1[..., :Cv], Wf2[..., :Cv]) and bool(torch.isnan(Wf2[..., Cv:]).all()) and not bool(torch.isnan(Wf2[..., :Cv]).any()), shape
        if wb:
            assert torch.equal(Wb1, Wb2) and not bool(torch.isnan(Wb2).any()), shape
