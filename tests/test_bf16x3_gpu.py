"""GPU: the 'bf16x3' precision (split-operand products on the bf16 matrix cores).

  * the split entry points against float64 torch: max error <= 2e-5 of sum |a*b| per output, and at least 50 x below the bf16 entry
    point's error on the same inputs (three products are really issued);
  * the library-built plans in bf16x3 against the reference goldens at the float32 tolerances of test_netplan_gpu.py;
  * the modules in bf16x3 bit-identical to the plans, the multi-stream step to the staged sequence;
  * the BASELINE shapes and the B = 32 canonical step against the oracle at the float32 tolerances;
  * the enhancement path: enhance_stream == enhance, within 1.5 LSB of float32 mode and closer to it than bf16 mode.
"""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import capi_nets as cn                                        # noqa: E402
from weights_recipe import digest, seeded_state_arrays        # noqa: E402

M = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'model.npz'))
PREC_BF16X3 = 2
EPI_NONE, EPI_BIAS, EPI_BIAS_LRELU, EPI_MASK_LRELU_GRAD, EPI_BIAS_EXPTANH = 0, 1, 2, 3, 4


def _lib():
    from nele_gan_amd import _lib as L
    from nele_gan_amd import ops  # noqa: F401  (declares the dense entry points)
    return L


def _geom(B, H, W, C, KH, KW, N):
    """valid convolution of a [B][H][W][C] buffer into a dense [B][Hout][Wout][N] one -> (ctypes geometry, M, Hout, Wout)"""
    Ho, Wo = H - KH + 1, W - KW + 1
    g = [H, W, C, 0, 0, Ho, Wo, KW * C, W * C, KH * KW * C, Ho, Wo, N, 0, 0]
    return (ctypes.c_int * 15)(*g), B * Ho * Wo, Ho, Wo


def _rel_err(got, ref, scale):
    return float(((got.double() - ref).abs() / scale.clamp_min(1e-30)).max())


def _conv_case(B, H, W, C, KH, KW, N, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    A = torch.randn((B, H, W, C), device='cuda', generator=g)
    Wt = torch.randn((N, C, KH, KW), device='cuda', generator=g) / np.sqrt(C * KH * KW)
    return A, Wt


def _fwd(L, A, Wt, x3, epi=EPI_NONE, bias=None, aux=None, slope=0.0):
    B, H, W, C = A.shape
    N, _, KH, KW = Wt.shape
    geom, Mrows, Ho, Wo = _geom(B, H, W, C, KH, KW, N)
    Wg = Wt.permute(0, 2, 3, 1).reshape(N, -1).contiguous()
    ne = int(L.lib.nele_weight_frag16_elems(N, KW * C, KH))
    out = torch.full((B, Ho, Wo, N), float('nan'), device='cuda')
    s = L.stream()
    bp, ap = (L.ptr(bias) if bias is not None else None), (L.ptr(aux) if aux is not None else None)
    if x3:
        if not L.lib.nele_conv_span_bf16x3_supported(Mrows, N, geom, KH, KW):
            return None
        hi = torch.empty(ne, dtype=torch.bfloat16, device='cuda')
        lo = torch.empty(ne, dtype=torch.bfloat16, device='cuda')
        L.call('nele_weight_prep_frag16x3', L.ptr(Wg), N, Wg.shape[1], KW * C, KH, L.ptr(hi), L.ptr(lo), s)
        L.call('nele_conv_span_bf16x3', L.ptr(A), L.ptr(hi), L.ptr(lo), bp, ap, L.ptr(out), Mrows, N, epi, slope, geom, KH, KW, A.numel(), s)
    else:
        if not L.lib.nele_conv_span_bf16_supported(Mrows, N, geom, KH, KW):
            return None
        wf = torch.empty(ne, dtype=torch.bfloat16, device='cuda')
        L.call('nele_weight_prep_frag16', L.ptr(Wg), N, Wg.shape[1], KW * C, KH, L.ptr(wf), s)
        L.call('nele_conv_span_bf16', L.ptr(A), L.ptr(wf), bp, ap, L.ptr(out), Mrows, N, epi, slope, geom, KH, KW, A.numel(), s)
    torch.cuda.synchronize()
    return out


def _wgrad(L, A, dO, KH, KW, x3):
    B, H, W, C = A.shape
    N = dO.shape[-1]
    geom, Mrows, Ho, Wo = _geom(B, H, W, C, KH, KW, N)
    nws = int(L.lib.nele_conv_wgrad_workspace_floats(Mrows, N, KH * KW * C, None))
    ws = torch.empty(nws, device='cuda')
    dW = torch.full((N, C, KH, KW), float('nan'), device='cuda')
    db = torch.empty(N, device='cuda')
    L.call('nele_conv_wgrad_bf16x3' if x3 else 'nele_conv_wgrad_bf16', L.ptr(A), L.ptr(dO), L.ptr(ws), nws, Mrows, N, geom, KH, KW, C, L.ptr(dW),
           L.ptr(db), 0, L.stream())
    torch.cuda.synchronize()
    return dW, db


# (C, N, KH, KW, H): G's Conv1d layers forward and their data-gradient geometries (channels swapped), D.layers.1-4 forward and data gradient
G_SHAPES = [(128, 256, 1, 5, 1), (256, 256, 1, 7, 1), (256, 64, 1, 5, 1), (256, 128, 1, 5, 1), (64, 256, 1, 5, 1)]
D_SHAPES = [(8, 16, 3, 3, 12), (16, 32, 5, 5, 14), (32, 48, 7, 7, 16), (48, 64, 9, 9, 18), (16, 8, 3, 3, 12), (32, 16, 5, 5, 14),
            (48, 32, 7, 7, 16)]


# EPI_BIAS_EXPTANH against exp(3.2 * tanh(x + bias)) in float64, x the EPI_NONE output of the same call.  The figures of the commit before the
# store epilogue became one helper were never measured, so the bound is the worst case of the float32 steps instead, each as a relative error
# of the result (= an absolute error of the exponent): the float32 add x + bias, half an ulp through 3.2 sech^2, at most 8e-8 (|v| in [1, 2));
# tanhf, 2 ulp of a value below 1, times 3.2: 3.8e-7; the product with 3.2f, half an ulp below 4: 1.2e-7; 3.2f against 3.2: 5e-8; expf, 1 ulp:
# 1.2e-7.  Sum 7.5e-7.  A wrong bias element or a missing tanh is off by tens of percent.
EXPTANH_ERR = 7.5e-7
# (C, N, KH, KW, Hout, B) at T = 40: a strip with two 64-channel chunks and a partial 128-position strip; a 2-D tile with a partial column
# tile and row tiles beyond Hout
EPI_CASES = {'strip': (64, 128, 1, 5, 1, 2), 'tile': (16, 32, 5, 5, 14, 1)}


@pytest.mark.parametrize('x3', [False, True])
@pytest.mark.parametrize('kind', ['strip', 'tile'])
def test_store_epilogues_equal_the_plain_output_post_processed(kind, x3):
    """EPI_BIAS, EPI_BIAS_LRELU and EPI_MASK_LRELU_GRAD are one float32 add and one select or multiply on the EPI_NONE output: bit for bit;
    EPI_BIAS_EXPTANH within the float32 rounding of its steps (EXPTANH_ERR)."""
    L = _lib()
    C, N, KH, KW, Ho, B = EPI_CASES[kind]
    A, Wt = _conv_case(B, Ho + KH - 1, 40 + KW - 1, C, KH, KW, N, 4242)
    g = torch.Generator(device='cuda').manual_seed(4243)
    bias = torch.randn(N, device='cuda', generator=g)
    plain = _fwd(L, A, Wt, x3)
    assert plain is not None and not torch.isnan(plain).any()
    aux = torch.randn(plain.shape, device='cuda', generator=g)
    slope = 0.3
    sl = torch.tensor(slope, dtype=torch.float32, device='cuda')
    vb = plain + bias
    assert torch.equal(_fwd(L, A, Wt, x3, EPI_BIAS, bias=bias), vb)
    assert torch.equal(_fwd(L, A, Wt, x3, EPI_BIAS_LRELU, bias=bias, slope=slope), torch.where(vb > 0, vb, sl * vb))
    assert torch.equal(_fwd(L, A, Wt, x3, EPI_MASK_LRELU_GRAD, aux=aux, slope=slope), torch.where(aux > 0, plain, sl * plain))
    ref = torch.exp(3.2 * torch.tanh(plain.double() + bias.double()))
    err = float(((_fwd(L, A, Wt, x3, EPI_BIAS_EXPTANH, bias=bias).double() - ref).abs() / ref).max())
    print('exptanh relative error', kind, x3, err)
    assert err <= EXPTANH_ERR, (kind, x3, err)


def test_n_chunk_walk_equals_one_workgroup_per_chunk():
    """bf16, C = 64 -> N = 128, k = 5, T = 32 at B = 256: 256 strips, so one workgroup per strip walks both 64-channel chunks; utterances 0
    and 255 must come out bit for bit as at B = 2, where every chunk has a workgroup of its own"""
    L = _lib()
    A, Wt = _conv_case(256, 1, 32 + 4, 64, 1, 5, 128, 777)
    big = _fwd(L, A, Wt, False)
    small = _fwd(L, A[[0, 255]].contiguous(), Wt, False)
    assert big is not None and small is not None and not torch.isnan(big).any()
    assert torch.equal(big[[0, 255]], small)


@pytest.mark.parametrize('T', [24, 40, 41, 77, 251, 501])
def test_split_conv_accuracy_against_float64(T):
    L = _lib()
    ran = 0
    for q, (C, N, KH, KW, H) in enumerate(G_SHAPES + D_SHAPES):
        B = 2 if KH == 1 else 1
        W = T + KW - 1
        A, Wt = _conv_case(B, H + KH - 1 if KH > 1 else 1, W, C, KH, KW, N, 1000 * T + q)
        ref = torch.nn.functional.conv2d(A.permute(0, 3, 1, 2).double(), Wt.double()).permute(0, 2, 3, 1)
        scale = torch.nn.functional.conv2d(A.permute(0, 3, 1, 2).double().abs(), Wt.double().abs()).permute(0, 2, 3, 1)
        o3 = _fwd(L, A, Wt, True)
        o1 = _fwd(L, A, Wt, False)
        if T >= 32 and (KH == 1 or KW * C <= 4096):
            assert o3 is not None, (C, N, KH, KW, T)        # the strip / tile kernels take every layer of the networks at T >= 32 but one
        if o3 is None:
            continue
        e3 = _rel_err(o3, ref, scale)
        assert e3 <= 2e-5, (C, N, KH, KW, T, e3)
        if o1 is not None:
            e1 = _rel_err(o1, ref, scale)
            assert e3 * 50 <= e1, (C, N, KH, KW, T, e3, e1)
            assert e1 <= 2 ** -7, (C, N, KH, KW, T, e1)     # bf16 rounding of both factors: at most 2^-8 each, relative to sum |a*b|
        ran += 1
        # weight gradient of the same layer: dOut of the output's shape
        dO = torch.randn(ref.shape, device='cuda', generator=torch.Generator(device='cuda').manual_seed(7 + q)).float().contiguous()
        Ad, dOd = A.permute(0, 3, 1, 2).double(), dO.permute(0, 3, 1, 2).double()
        rW = torch.nn.grad.conv2d_weight(Ad, Wt.shape, dOd)
        sW = torch.nn.grad.conv2d_weight(Ad.abs(), Wt.shape, dOd.abs())
        w3, b3 = _wgrad(L, A, dO, KH, KW, True)
        w1, _ = _wgrad(L, A, dO, KH, KW, False)
        ew3, ew1 = _rel_err(w3, rW, sW), _rel_err(w1, rW, sW)
        assert ew3 <= 2e-5, ('wgrad', C, N, KH, KW, T, ew3)
        assert ew3 * 50 <= ew1, ('wgrad', C, N, KH, KW, T, ew3, ew1)
        assert ew1 <= 2 ** -7, ('wgrad', C, N, KH, KW, T, ew1)
        np.testing.assert_allclose(b3.cpu().numpy(), dO.double().sum((0, 1, 2)).cpu().numpy(), rtol=1e-4, atol=1e-3)
    assert ran >= (len(G_SHAPES) + len(D_SHAPES) - 1 if T >= 32 else 0)


def test_split_wgrad_kernel_takes_the_network_layers():
    """the weight gradients of G's conv layers and of D.layers.1-4 at T = 251 run on the split tile kernel (not on the float32 fallback)"""
    L = _lib()
    for C, N, KH, KW, H in G_SHAPES[:3] + D_SHAPES[:4]:
        geom, Mrows, _, _ = _geom(2, H + KH - 1 if KH > 1 else 1, 251 + KW - 1, C, KH, KW, N)
        assert L.lib.nele_conv_wgrad_bf16x3_supported(Mrows, N, geom, KH, KW) == 1, (C, N, KH, KW)


def check_grad(prefix, name, g, rtol=3e-4):
    g = g.detach().cpu().numpy()
    if prefix + name in M:
        ref = M[prefix + name]
        np.testing.assert_allclose(g, ref.reshape(g.shape), rtol=rtol, atol=2e-5 * np.abs(ref).max())
    else:
        s, a, smp = digest(g)
        ra = float(M[prefix + name + '#abs'])
        assert s == pytest.approx(float(M[prefix + name + '#sum']), rel=1e-3, abs=2e-5 * ra)
        assert a == pytest.approx(ra, rel=2e-4)
        ref = M[prefix + name + '#smp']
        np.testing.assert_allclose(smp, ref, rtol=1e-3, atol=2e-5 * np.abs(ref).max())


# Measured on the golden generator input: the gradients of layers 1 and 0 (convolutions.1, .0) differ from the golden by up to 4.6e-2 of a
# layer's largest element (median 1.8e-4), every other gradient and the mask by ~1e-5; with only layer 1's forward on the float32 kernel
# all of them agree to 1e-5, and no backward kernel choice changes it.  A ~1e-5 change of layer 1's output that moves the backward pass
# this much is a LeakyReLU input sitting at the kink (its derivative 1 or 0.3), spread over the channels of the later frames by the
# cumulative layer norm's backward.  Those two layers are checked on their sum of magnitudes at 2e-3, the rest at float32's tolerances.
KINK_LAYERS = ('convolutions.0.', 'convolutions.1.')


def test_generator_plans_in_bf16x3_match_reference_golden():
    st = seeded_state_arrays(cn.g_keys_shapes(), 101)
    G = cn.CapiGenerator(2, 40, st, bf16=PREC_BF16X3)
    x, y = torch.from_numpy(M['x']).cuda(), torch.from_numpy(M['y']).cuda()
    mask = G.forward(x, y)
    np.testing.assert_allclose(mask.cpu().numpy(), M['g_mask'], rtol=1e-4)
    G.backward(torch.from_numpy(M['g_gw']).cuda().contiguous(), mask)
    torch.cuda.synchronize()
    for k in G.names:
        if k.startswith(KINK_LAYERS):
            g = G.grad_of(k).detach().cpu().numpy()
            s, a, _ = digest(g)
            ra = float(M['g_grad.' + k + '#abs']) if 'g_grad.' + k + '#abs' in M else float(np.abs(M['g_grad.' + k]).sum())
            assert a == pytest.approx(ra, rel=2e-3), k
        else:
            check_grad('g_grad.', k, G.grad_of(k))
    G.close()


@pytest.mark.parametrize('train', [False, True])
def test_discriminator_plans_in_bf16x3_match_reference_golden(train):
    st = seeded_state_arrays(cn.d_keys_shapes(3, 3), 202)
    x = torch.from_numpy(M['d_in']).cuda()
    B, _, _, T = x.shape
    din = torch.zeros((B, 64, T, 4), device='cuda')
    din[..., :3] = x.permute(0, 2, 3, 1)
    D = cn.CapiDiscriminator(B, T, st, train=train, bf16=PREC_BF16X3)
    sc = D.forward(din)
    pre = 'd_train_' if train else 'd_eval_'
    np.testing.assert_allclose(sc.cpu().numpy(), M[pre + 'score'], rtol=2e-5)
    tgt = torch.from_numpy(M['d_tgt']).cuda()
    dscore = (2.0 * (sc - tgt) / sc.numel()).contiguous()
    D.backward(dscore, sc, din)
    torch.cuda.synchronize()
    if train:
        for k, t in zip(D.uv_names, D.uv):
            np.testing.assert_allclose(t.cpu().numpy(), M['d_train_buf.' + k], rtol=2e-5, atol=1e-7)
    for k in D.pnames:
        check_grad(pre + 'grad.', k, D.grad_of(k), rtol=2e-3)
    ref = M[pre + 'din_grad']
    got = D.ddin()[..., :3].permute(0, 3, 1, 2).cpu().numpy()
    np.testing.assert_allclose(got, ref, rtol=2e-3, atol=2e-5 * np.abs(ref).max())
    D.close()


def _load(module, seed):
    sd = module.state_dict()
    arrs = seeded_state_arrays([(k, tuple(v.shape)) for k, v in sd.items()], seed)
    module.load_state_dict({k: torch.from_numpy(v) for k, v in arrs.items()})
    return module.cuda()


def test_discriminator_quality_eval_in_bf16x3():
    from nele_gan_amd import model
    Q = _load(model.Discriminator_Quality(), 303)
    Q.precision = 'bf16x3'
    Q.eval()
    with torch.no_grad():
        sc = Q(torch.from_numpy(M['d_in'][:, [0, 2]].copy()).cuda())
    np.testing.assert_allclose(sc.cpu().numpy(), M['dq_eval_score'], rtol=2e-5)


@pytest.mark.parametrize('B,T', [(2, 40), (8, 251), (1, 300)])
def test_generator_module_is_bit_identical_to_the_plans(B, T):
    from nele_gan_amd import model
    st = seeded_state_arrays(cn.g_keys_shapes(), 101)
    g = torch.Generator(device='cuda').manual_seed(B * 1000 + T)
    x = torch.rand((B, T, 64), device='cuda', generator=g) + 0.1
    y = torch.rand((B, T, 64), device='cuda', generator=g) + 0.1
    gw = torch.randn((B, T, 64), device='cuda', generator=g)
    Gm = model.Generator_Conv1D_cLN()
    Gm.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    Gm = Gm.cuda()
    Gm.precision = 'bf16x3'
    Gm.flat_parameters().grad.zero_()
    mask_m = Gm(x, y)
    (mask_m * gw).sum().backward()
    Gc = cn.CapiGenerator(B, T, st, bf16=PREC_BF16X3)
    for rep in range(2):
        Gc.grad.zero_()
        mask_c = Gc.forward(x, y)
        Gc.backward(gw, mask_c)
        torch.cuda.synchronize()
        assert torch.equal(mask_c, mask_m.detach())
        assert torch.equal(Gc.grad, Gm.flat_parameters().grad)
    Gc.close()


@pytest.mark.parametrize('B,T,cin,nout', [(2, 40, 3, 3), (8, 251, 3, 3), (4, 128, 2, 2)])
def test_discriminator_module_is_bit_identical_to_the_plans(B, T, cin, nout):
    from nele_gan_amd import model
    st = seeded_state_arrays(cn.d_keys_shapes(cin, nout), 202)
    Dm = model.Discriminator(nout=nout) if cin == 3 else model.Discriminator_Quality(nout=nout)
    Dm.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    Dm = Dm.cuda()
    Dm.precision = 'bf16x3'
    Dm.train()
    g = torch.Generator(device='cuda').manual_seed(B * 1000 + T)
    din = torch.zeros((B, 64, T, 4), device='cuda')
    din[..., :cin] = torch.rand((B, 64, T, cin), device='cuda', generator=g)
    tgt = torch.rand((B, nout), device='cuda', generator=g)
    dm = din.clone().requires_grad_(True)
    Dm.flat_parameters().grad.zero_()
    sc_m = Dm.forward_packed(dm)
    torch.nn.functional.mse_loss(sc_m, tgt).backward()
    Dc = cn.CapiDiscriminator(B, T, st, cin=cin, nout=nout, bf16=PREC_BF16X3, train=True)
    for rep in range(2):
        if rep:
            Dc.grad.zero_()
        sc_c = Dc.forward(din)
        dscore = (2.0 * (sc_c - tgt) / sc_c.numel()).contiguous()
        Dc.backward(dscore, sc_c, din)
        torch.cuda.synchronize()
        if rep == 0:
            assert torch.equal(sc_c, sc_m.detach())
            assert torch.equal(Dc.grad, Dm.flat_parameters().grad)
            assert torch.equal(Dc.ddin(), dm.grad)
            for k, t in zip(Dc.uv_names, Dc.uv):
                assert torch.equal(t, Dm.state_dict()[k])
    Dc.close()


@pytest.mark.parametrize('B,T', [(32, 251), (4, 501)])
def test_generator_discriminator_at_baseline_frame_counts_bf16x3(B, T):
    """G -> energy normalisation -> D -> MSE in bf16x3 against oracle/nets.py at the float32 tolerances of test_step_parity_gpu.py"""
    from nele_gan_amd import model as mods
    from oracle import nets
    rs = np.random.RandomState(B * 1000 + T)
    G = _load(mods.Generator_Conv1D_cLN(), 7)
    D = _load(mods.Discriminator(nout=2), 8)
    G.precision = D.precision = 'bf16x3'
    x = (0.1 + 0.4 * rs.rand(B, T, 64)).astype(np.float32)
    y = (0.1 + 0.4 * rs.rand(B, T, 64)).astype(np.float32)
    tgt = rs.rand(B, 2).astype(np.float32)
    sdg = {k: t.detach().cpu().clone().requires_grad_(True) for k, t in G.state_dict().items()}
    sdd = {k: t.detach().cpu().clone().requires_grad_(not (k.endswith('_u') or k.endswith('_v'))) for k, t in D.state_dict().items()}
    xo, yo = torch.from_numpy(x), torch.from_numpy(y)
    mo = nets.generator_forward(sdg, xo, yo)
    eo, b2o = nets.energy_norm(mo, xo)
    so, _ = nets.discriminator_forward(sdd, nets.d_inputs(eo, yo, xo), train=True)
    lo = torch.nn.functional.mse_loss(so, torch.from_numpy(tgt))
    lo.backward()
    D.train()
    G.flat_parameters().grad.zero_()
    D.flat_parameters().grad.zero_()
    xc, yc = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    m = G(xc, yc)
    din, b2 = mods.energy_norm_pack(m, xc, yc)
    s = D.forward_packed(din)
    loss = torch.nn.functional.mse_loss(s, torch.from_numpy(tgt).cuda())
    loss.backward()
    torch.cuda.synchronize()
    mh, sh = m.detach().cpu().numpy(), s.detach().cpu().numpy()
    np.testing.assert_allclose(mh, mo.detach().numpy(), rtol=3e-4)
    np.testing.assert_allclose(b2.cpu().numpy(), b2o.detach().numpy(), rtol=1e-4)
    np.testing.assert_allclose(sh, so.detach().numpy(), rtol=1e-4)
    assert float(loss) == pytest.approx(float(lo), rel=1e-4)
    for name, mod, sd in (('G', G, sdg), ('D', D, sdd)):
        for k, p in mod.named_parameters():
            ref = sd[k].grad.numpy()
            np.testing.assert_allclose(p.grad.cpu().numpy(), ref, rtol=5e-3, atol=2e-4 * np.abs(ref).max(), err_msg=name + ' ' + k)


def _trainer(metrics, precision, seed=666):
    from nele_gan_amd.train_nele import GanTrainer
    tr = GanTrainer(metrics, seed=seed)
    tr.G.precision = precision
    tr.D.precision = precision
    return tr


def _state(module):
    return {k: t.detach().cpu().clone() for k, t in module.state_dict().items()}


def test_baseline_step_b32_against_the_oracle_bf16x3():
    """B = 32, L = 64 000, SIIB + ESTOI: the multi-stream step in bf16x3 against oracle.step.CpuStep at the float32 tolerances"""
    from nele_gan_amd import synth
    from oracle.step import CpuStep
    B, L = 32, 64000
    c, v = synth.batch(B, L, start=0)
    cw, nw = torch.from_numpy(c).cuda(), torch.from_numpy(v).cuda()
    tr = _trainer('siib&estoi', 'bf16x3')
    cpu = CpuStep(_state(tr.G), _state(tr.D), metrics=('siib', 'estoi'))
    lg, ld, tgt = tr.canonical_step(cw, nw)
    torch.cuda.synchronize()
    enh_h = tr._last_enh.cpu().numpy()
    assert all(x == 0 for x in tr.check_status().values())
    cb, cm, cp, nb = cpu.features(c, v)
    lg_ref = cpu.g_step(cb, nb)
    enh_ref = cpu.generate(cb, nb, cm, cp)
    ld_ref = cpu.d_step([e for e in enh_h], nb, cb, tgt.cpu().numpy())
    assert float(lg) == pytest.approx(lg_ref, rel=1e-4)
    assert float(ld) == pytest.approx(ld_ref, rel=5e-4)
    for b in range(B):
        d = np.abs(enh_h[b] - enh_ref[b])
        assert d.max() <= 1.5 / 32768 and np.mean(d > 1e-7) < 0.02
    for k, t in tr.G.state_dict().items():
        np.testing.assert_allclose(t.cpu().numpy(), cpu.g[k].detach().numpy(), rtol=1e-3, atol=2e-5, err_msg=k)


def test_multistream_step_is_bit_identical_to_the_staged_sequence_bf16x3():
    from nele_gan_amd import synth
    c, v = synth.batch(3, 24000, start=40)
    cw, nw = torch.from_numpy(c).cuda(), torch.from_numpy(v).cuda()
    a = _trainer('siib&haspi&estoi', 'bf16x3')
    b = _trainer('siib&haspi&estoi', 'bf16x3')
    for step in range(2):
        lg_a, ld_a, tgt_a = a.canonical_step(cw, nw)
        f = b.features(cw, nw)
        lg_b = b.g_step(f['clean_band'], f['noise_band'])
        enh_b = b.generate(f['clean_band'], f['noise_band'], f['clean_spec'])
        tgt_b = b.true_metrics(cw, enh_b, nw)
        ld_b = b.d_step(b.d_inputs(enh_b, f['noise_band'], f['clean_band']), tgt_b)
        torch.cuda.synchronize()
        assert torch.equal(a._last_enh, enh_b), step
        assert torch.equal(tgt_a, tgt_b), step
        assert float(lg_a) == float(lg_b) and float(ld_a) == float(ld_b), step
        assert torch.equal(a.G.flat_parameters().flat, b.G.flat_parameters().flat), step
        assert torch.equal(a.D.flat_parameters().flat, b.D.flat_parameters().flat), step
    assert all(x == 0 for x in a.check_status().values())


def test_enhancement_in_bf16x3():
    from nele_gan_amd import synth
    from nele_gan_amd.inference import Enhancer
    B, L = 4, 128000
    c, v = synth.batch(B, L, start=900)
    cw, nw = torch.from_numpy(c).cuda(), torch.from_numpy(v).cuda()
    torch.manual_seed(3)
    e = Enhancer()
    outs = {}
    for prec in ('f32', 'bf16', 'bf16x3'):
        e.G.precision = prec
        outs[prec] = e.enhance(cw, nw, pcm16=True).clone()
    e.G.precision = 'bf16x3'
    streamed = list(e.enhance_stream([(cw, nw), (cw[:2], nw[:2])], inflight=2))
    assert torch.equal(streamed[0], outs['bf16x3']) and torch.equal(streamed[1], e.enhance(cw[:2], nw[:2]))
    shared = Enhancer(G=e.G)                                  # a generator handed in: layouts rewritten per call
    assert torch.equal(shared.enhance(cw, nw), outs['bf16x3'])
    assert torch.equal(list(shared.enhance_stream([(cw, nw)], inflight=2))[0], outs['bf16x3'])
    d3 = (outs['bf16x3'] - outs['f32']).abs()
    d1 = (outs['bf16'] - outs['f32']).abs()
    assert float(d3.max()) <= 1.5 / 32768
    assert not torch.equal(outs['bf16x3'], outs['f32'])       # the split kernels ran: not a silent float32 fallback
    assert float(d3.max()) < float(d1.max())
