"""GPU: the causal (prefix) energy normalisation as a `norm` mode of the offline and training paths (csrc/prefixnorm.hip,
model.energy_norm_pack / normed_alpha2, GanTrainer, Enhancer) - the same arithmetic as the real-time path bit for bit, forward and
gradient against the float64 restatement (tests/prefix_norm_ref.py), edge frames, batch invariance, and the default path untouched."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import prefix_norm_ref as ref  # noqa: E402
from test_realtime_gpu import HOP, G, f32_run, load_recipe, utts  # noqa: E402,F401  (the real-time suite's fixtures: generator, four utterances, one f32 streamed run)

P, INV_P = 1.0 / 6, 6.0


@pytest.fixture(scope='module')
def mods():
    from nele_gan_amd import model
    return model


def _kernel_inputs(B, T, seed, zero_head=0, frames=None):
    """random band features as in test_models_vs_oracle_other_shapes, a mask in exp(3.2 tanh)'s range, a random d(din); the first
    ``zero_head`` frames and the frames behind ``frames[b]`` are exact zeros, as the feature kernels leave them"""
    rs = np.random.RandomState(seed)
    clean = (0.1 + 0.4 * rs.rand(B, T, 64)).astype(np.float32)
    noise = (0.1 + 0.4 * rs.rand(B, T, 64)).astype(np.float32)
    mask = np.exp(3.2 * np.tanh(rs.randn(B, T, 64))).astype(np.float32)
    ddin = rs.randn(B, 64, T, 4).astype(np.float32)
    clean[:, :zero_head] = 0
    noise[:, :zero_head] = 0
    if frames is not None:
        for b, n in enumerate(frames):
            clean[b, n:] = 0
            noise[b, n:] = 0
    return [torch.from_numpy(a).cuda() for a in (clean, mask, noise, ddin)]


def _run_kernels(clean, mask, noise, ddin, with_din=True):
    from nele_gan_amd import ops
    ratio, s2, din, alpha2 = ops.energy_norm_prefix_fwd(clean, mask, noise, P, INV_P, want_din=True, want_alpha2=True)
    dmask = ops.energy_norm_prefix_bwd(clean, mask, ratio, s2, ddin, P, INV_P, din=din if with_din else None)
    torch.cuda.synchronize()
    return ratio, s2, din, alpha2, dmask


def _closed_form64(clean, mask, ddin):
    dE = ddin[..., 0].permute(0, 2, 1).double().cpu()
    return ref.prefix_dmask_closed_form(mask.double().cpu(), clean.double().cpu(), dE)


# ---------------------------------------------------------------- 1. the real-time arithmetic, bit for bit
def test_alpha2_is_bit_identical_to_the_real_time_path(mods, utts, f32_run):
    _, dbg, _ = f32_run
    cl, _ = utts
    for i, c in enumerate(cl):
        T = 1 + len(c) // HOP
        band = dbg.band[i, :T].unsqueeze(0).contiguous()
        mask = dbg.mask[i, :T].unsqueeze(0).contiguous()
        a2 = mods.normed_alpha2(mask, band, norm='prefix')
        assert a2.shape == (1, T, 64)
        assert torch.equal(a2[0], dbg.alpha2[i, :T]), i


# ---------------------------------------------------------------- 2. offline = streamed signal
def test_offline_prefix_enhancer_equals_the_streamed_output(G, utts, f32_run):
    from nele_gan_amd.inference import Enhancer
    _, _, ys = f32_run
    cl, ns = utts
    G.precision = 'f32'
    e = Enhancer(G=G, norm='prefix')
    for i, (c, n) in enumerate(zip(cl, ns)):
        y = e.enhance(torch.from_numpy(c).cuda().reshape(1, -1), torch.from_numpy(n).cuda().reshape(1, -1), pcm16=False, rms_target=0)[0]
        assert y.shape == ys[i].shape == (HOP * (len(c) // HOP),)
        err, peak = (y - ys[i]).abs().max().item(), ys[i].abs().max().item()
        print('utterance %d: max |offline - streamed| = %.3e of peak' % (i, err / peak))
        assert err <= 1e-4 * peak


# ---------------------------------------------------------------- 3. forward and gradient parity
@pytest.mark.parametrize('B,T,frames', [(3, 57, None), (1, 132, None), (3, 90, (90, 41, 66))])
def test_forward_and_gradients_vs_float64_restatement(mods, B, T, frames):
    """the G-step chain G -> prefix normalisation -> D -> MSE against oracle.nets + the restatement in float64 (a padded batch: the
    oracle runs every utterance alone over its own frames); tolerances of test_models_vs_oracle_other_shapes"""
    rs = np.random.RandomState(B * 100 + T)
    Gm = load_recipe(mods.Generator_Conv1D_cLN(), 7)
    D = load_recipe(mods.Discriminator(nout=2), 8)
    x = (0.1 + 0.4 * rs.rand(B, T, 64)).astype(np.float32)
    y = (0.1 + 0.4 * rs.rand(B, T, 64)).astype(np.float32)
    tgt = rs.rand(B, 2).astype(np.float32)
    fr = list(frames) if frames is not None else [T] * B
    for b, n in enumerate(fr):
        x[b, n:] = 0
        y[b, n:] = 0
    # oracle, float64
    sdg = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in Gm.state_dict().items()}
    sdd = {k: v.detach().cpu().double().clone() for k, v in D.state_dict().items()}
    scores, ratios, dins = [], [], []
    for b, n in enumerate(fr):
        xo, yo = torch.from_numpy(x[b:b + 1, :n]).double(), torch.from_numpy(y[b:b + 1, :n]).double()
        mo = ref.generator_forward(sdg, xo, yo)
        eo, ro = ref.prefix_energy_norm(mo, xo)
        d_in = ref.d_inputs(eo, yo, xo)
        so, _ = ref.discriminator_forward(sdd, d_in, train=True)
        scores.append(so)
        ratios.append(ro.detach()[0])
        dins.append(d_in.detach()[0])
    so = torch.cat(scores)
    torch.nn.functional.mse_loss(so, torch.from_numpy(tgt).double()).backward()
    # HIP
    D.train()
    Gm.flat_parameters().grad.zero_()
    D.flat_parameters().grad.zero_()
    xc, yc = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    m = Gm(xc, yc)
    din, ratio = mods.energy_norm_pack(m, xc, yc, norm='prefix')
    assert ratio.shape == (B, T) and din.shape == (B, 64, T, 4)
    fr_t = None if frames is None else torch.tensor(fr, dtype=torch.int32).cuda()
    s = D.forward_packed(din, fr_t)
    loss = torch.nn.functional.mse_loss(s, torch.from_numpy(tgt).cuda())
    loss.backward()
    torch.cuda.synchronize()
    got = din.detach().cpu().numpy()
    for b, n in enumerate(fr):
        np.testing.assert_allclose(ratio[b, :n].cpu().numpy(), ratios[b].numpy(), rtol=1e-4)
        np.testing.assert_allclose(np.transpose(got[b, :, :n, :3], (2, 0, 1)), dins[b].numpy(), rtol=1e-4)
        assert np.all(got[b, :, n:, :] == 0) and np.all(got[b, :, :, 3] == 0)
    np.testing.assert_allclose(s.detach().cpu().numpy(), so.detach().numpy(), rtol=1e-4)
    for k, p in Gm.named_parameters():
        g = sdg[k].grad.numpy()
        np.testing.assert_allclose(p.grad.cpu().numpy(), g, rtol=5e-3, atol=1e-4 * np.abs(g).max(), err_msg='G ' + k)


@pytest.mark.parametrize('with_din', [True, False])
@pytest.mark.parametrize('B,T', [(3, 57), (1, 132), (2, 600)])
def test_backward_kernel_alone_vs_closed_form(B, T, with_din):
    """dmask of nele_energy_norm_prefix_bwd on a random d(din) against the closed form in float64, bounded as the existing backward
    kernel is through test_models_vs_oracle_other_shapes (rtol 5e-3, atol 1e-4 of the peak).  That bound holds for the restatement
    itself evaluated in float32 on the CPU on these inputs: its largest error against float64 is 1.0e-7, 1.1e-7 and 1.7e-7 of the peak
    for the three shapes (measured, torch float32 against float64), so no wider bound is needed.  T = 600 takes
    the kernels over their 512-frame chunk boundary."""
    clean, mask, noise, ddin = _kernel_inputs(B, T, 11 * B + T)
    ratio, s2, din, alpha2, dmask = _run_kernels(clean, mask, noise, ddin, with_din)
    want = _closed_form64(clean, mask, ddin).numpy()
    r64, _, s264 = ref.prefix_ratio(mask.double().cpu(), clean.double().cpu())
    np.testing.assert_allclose(ratio.cpu().numpy(), r64.numpy(), rtol=1e-6)
    # every term of S2 is mask times the float32 nearest to clean^6 (the arithmetic contract): half an ulp of float32 per term at most
    np.testing.assert_allclose(s2.cpu().numpy(), s264.numpy(), rtol=2.0 ** -24)
    err = np.abs(dmask.cpu().numpy() - want).max() / np.abs(want).max()
    print('B %d T %d din %s: max |dmask - float64| = %.3e of peak' % (B, T, with_din, err))
    np.testing.assert_allclose(dmask.cpu().numpy(), want, rtol=5e-3, atol=1e-4 * np.abs(want).max())


# ---------------------------------------------------------------- 4. edge frames
def test_leading_zero_frames_and_padded_rows(mods):
    B, T, k = 3, 90, 4
    frames = (90, 41, 66)
    clean, mask, noise, ddin = _kernel_inputs(B, T, 5, zero_head=k, frames=frames)
    for with_din in (True, False):
        ratio, s2, din, alpha2, dmask = _run_kernels(clean, mask, noise, ddin, with_din)
        for t in (ratio, s2, din, alpha2, dmask):
            assert torch.isfinite(t).all()
        assert torch.equal(ratio[:, :k], torch.ones_like(ratio[:, :k])) and float(s2[:, :k].abs().max()) == 0.0
        assert torch.equal(alpha2[:, :k], mask[:, :k])
        assert float(din[:, :, :k].abs().max()) == 0.0 and float(dmask[:, :k].abs().max()) == 0.0
        for b, n in enumerate(frames):
            assert float(din[b, :, n:].abs().max()) == 0.0 if n < T else True
            assert float(dmask[b, n:].abs().max()) == 0.0 if n < T else True
            # the sums stop growing behind the utterance's end
            assert torch.equal(s2[b, n - 1:], s2[b, n - 1].expand(T - n + 1)) and torch.equal(ratio[b, n - 1:], ratio[b, n - 1].expand(T - n + 1))
        want = _closed_form64(clean, mask, ddin).numpy()
        np.testing.assert_allclose(dmask.cpu().numpy(), want, rtol=5e-3, atol=1e-4 * np.abs(want).max())
    # through autograd: the zero frames' gradient is exactly zero, nothing is NaN
    m = mask.clone().requires_grad_(True)
    d, _ = mods.energy_norm_pack(m, clean, noise, norm='prefix')
    (d * ddin).sum().backward()
    assert torch.isfinite(m.grad).all() and float(m.grad[:, :k].abs().max()) == 0.0


# ---------------------------------------------------------------- 5. batch invariance
def test_a_row_does_not_depend_on_the_batch():
    T = 57
    clean, mask, noise, ddin = _kernel_inputs(256, T, 9)
    row = 0
    one = _run_kernels(*[t[row:row + 1].contiguous() for t in (clean, mask, noise, ddin)])
    # the same utterance in the middle of B = 50 and of B = 256
    for Bn, pos in ((50, 23), (256, 131)):
        sel = list(range(1, Bn))
        sel.insert(pos, row)
        idx = torch.tensor(sel).cuda()
        many = _run_kernels(*[t[idx].contiguous() for t in (clean, mask, noise, ddin)])
        for a, b, name in zip(one, many, ('ratio', 's2', 'din', 'alpha2', 'dmask')):
            assert torch.equal(a[0], b[pos]), (Bn, name)


# ---------------------------------------------------------------- 6. the mode reaches every path
def test_prefix_trainer_step_generate_and_checkpoints(mods, tmp_path):
    from nele_gan_amd import audio_util as au
    from nele_gan_amd import synth
    from nele_gan_amd.inference import Enhancer
    from nele_gan_amd.train_nele import GanTrainer
    c, v = synth.batch(8, 16000, start=900)
    cw, nw = torch.from_numpy(c).cuda(), torch.from_numpy(v).cuda()
    tr = GanTrainer('siib&estoi', pcm16=False, norm='prefix')
    lg, ld, tgt = tr.canonical_step(cw, nw)
    torch.cuda.synchronize()
    assert np.isfinite(float(lg)) and np.isfinite(float(ld)) and torch.isfinite(tgt).all()
    st = tr.check_status()
    assert all(st[k] == 0 for k in ('siib_undefined', 'haspi_below_threshold', 'skipped_g_steps', 'skipped_d_steps')), st
    enh = tr._last_enh
    f = tr.features(cw, nw)
    with torch.no_grad():
        mask = tr.G(f['clean_band'], f['noise_band'])
    a2 = ref.prefix_alpha2(mask.double(), f['clean_band'].double()).float()
    want = au.gain_istft(a2, f['clean_spec'], rms_target=0, pcm16=False)
    assert enh.shape == want.shape
    assert (enh - want).abs().max().item() <= 1e-6 * want.abs().max().item()
    # same weights, utterance-level trainer: another waveform
    tu = GanTrainer('siib&estoi', pcm16=False)
    assert tu.norm == 'utterance'
    tu.G.load_state_dict(tr.G.state_dict())
    enh_u = tu.generate(f['clean_band'], f['noise_band'], f['clean_spec'])
    enh_p = tr.generate(f['clean_band'], f['noise_band'], f['clean_spec'])
    assert torch.equal(enh_p, enh)
    assert not torch.equal(enh_u, enh_p) and (enh_u - enh_p).abs().max().item() > 1e-3 * enh_p.abs().max().item()
    # checkpoints
    pp, pu = str(tmp_path / 'prefix.pt'), str(tmp_path / 'utt.pt')
    tr.save_checkpoint(pp)
    tu.save_checkpoint(pu)
    assert torch.load(pp, map_location='cpu')['enhance-norm'] == 'prefix'
    assert sorted(torch.load(pu, map_location='cpu').keys()) == ['enhance-model', 'intel-model']
    assert Enhancer(pp).norm == 'prefix' and Enhancer(pu).norm == 'utterance'
    assert Enhancer(pp, norm='utterance').norm == 'utterance' and Enhancer(pu, norm='prefix').norm == 'prefix'
    with pytest.raises(ValueError):
        tu.load_checkpoint(pp)
    with pytest.raises(ValueError):
        tr.load_checkpoint(pu)
    tr.load_checkpoint(pp)
    tu.load_checkpoint(pp, allow_norm_mismatch=True)
    # the offline enhancer in the checkpoint's mode, without the final gain: the trainer's signal
    out = Enhancer(pp).enhance(cw, nw, pcm16=False, rms_target=0)
    assert (out - enh).abs().max().item() <= 1e-6 * enh.abs().max().item()


# ---------------------------------------------------------------- 7. default path untouched
def test_default_mode_is_the_old_entry_points_bit_for_bit(mods):
    from nele_gan_amd import ops
    clean, mask, noise, _ = _kernel_inputs(3, 57, 21)
    beta2, s2, din, alpha2 = ops.energy_norm_fwd(clean, mask, noise, P, INV_P, want_din=True, want_alpha2=True)
    d0, b0 = mods.energy_norm_pack(mask, clean, noise)
    d1, b1 = mods.energy_norm_pack(mask, clean, noise, norm='utterance')
    assert torch.equal(d0, din) and torch.equal(b0, beta2) and torch.equal(d1, din) and torch.equal(b1, beta2)
    assert b0.shape == (3,)
    assert torch.equal(mods.normed_alpha2(mask, clean), alpha2) and torch.equal(mods.normed_alpha2(mask, clean, norm='utterance'), alpha2)
    assert not torch.equal(mods.normed_alpha2(mask, clean, norm='prefix'), alpha2)


def test_default_trainer_step_is_unchanged_by_a_prefix_trainer_in_the_process():
    from nele_gan_amd import synth
    from nele_gan_amd.train_nele import GanTrainer
    c, v = synth.batch(4, 16000, start=950)
    cw, nw = torch.from_numpy(c).cuda(), torch.from_numpy(v).cuda()

    def default_step():
        tr = GanTrainer('siib&estoi')
        f = tr.features(cw, nw)
        lg = float(tr.g_step(f['clean_band'], f['noise_band']))
        enh = tr.generate(f['clean_band'], f['noise_band'], f['clean_spec'])
        torch.cuda.synchronize()
        return lg, enh

    lg0, enh0 = default_step()
    tp = GanTrainer('siib&estoi', norm='prefix')
    fp = tp.features(cw, nw)
    lgp = float(tp.g_step(fp['clean_band'], fp['noise_band']))
    tp.generate(fp['clean_band'], fp['noise_band'], fp['clean_spec'])
    lg1, enh1 = default_step()
    assert lg0 == lg1 and torch.equal(enh0, enh1)
    assert lgp != lg0
