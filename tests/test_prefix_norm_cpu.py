"""CPU: the float64 restatement of the prefix energy normalisation (tests/prefix_norm_ref.py) against the utterance-level oracle and
against its own autograd (the closed-form gradient the backward kernel implements), and the `norm` argument's error behaviour."""
import numpy as np
import pytest
import torch

from prefix_norm_ref import prefix_dmask_closed_form, prefix_energy_norm, prefix_ratio


def _features(B, T, seed, zero_frames=()):
    rs = np.random.RandomState(seed)
    clean = torch.from_numpy(0.1 + 0.4 * rs.rand(B, T, 64))
    mask = torch.from_numpy(np.exp(3.2 * np.tanh(rs.randn(B, T, 64))))
    for t in zero_frames:
        clean[:, t] = 0.0
    return clean, mask


def test_last_frame_ratio_is_the_utterance_level_beta2():
    from oracle import nets
    clean, mask = _features(3, 57, 1)
    ratio, s1, s2 = prefix_ratio(mask, clean)
    _, beta2 = nets.energy_norm(mask, clean)
    np.testing.assert_allclose(ratio[:, -1].numpy(), beta2.numpy(), rtol=1e-13)
    # energy preserved over every prefix
    np.testing.assert_allclose((ratio * s2).numpy(), s1.numpy(), rtol=1e-13)


@pytest.mark.parametrize('zero_frames', [(), (0, 1, 2), (0, 1, 9, 10, 30)])
def test_closed_form_gradient_equals_autograd(zero_frames):
    clean, mask = _features(2, 41, 2, zero_frames)
    rs = np.random.RandomState(3)
    dE = torch.from_numpy(rs.randn(2, 41, 64))
    m = mask.clone().requires_grad_(True)
    enh, ratio = prefix_energy_norm(m, clean)
    (enh * dE).sum().backward()
    got = prefix_dmask_closed_form(mask, clean, dE)
    assert torch.isfinite(m.grad).all() and torch.isfinite(got).all()
    np.testing.assert_allclose(got.numpy(), m.grad.numpy(), rtol=1e-12, atol=1e-12 * float(m.grad.abs().max()))
    for t in zero_frames:
        assert float(got[:, t].abs().max()) == 0.0
    if zero_frames and zero_frames[0] == 0:
        k = 1 + max(i for i in range(len(zero_frames)) if zero_frames[i] == i)      # leading all-zero frames: S2 = 0
        assert float((ratio.detach()[:, :k] - 1.0).abs().max()) == 0.0


def test_unknown_norm_raises():
    from nele_gan_amd import model
    from nele_gan_amd.inference import Enhancer
    from nele_gan_amd.train_nele import GanTrainer
    x = torch.zeros(1, 30, 64)
    with pytest.raises(ValueError):
        model.energy_norm_pack(x, x, x, norm='bogus')
    with pytest.raises(ValueError):
        model.normed_alpha2(x, x, norm='bogus')
    with pytest.raises(ValueError):
        GanTrainer('siib&estoi', device='cpu', norm='bogus')
    with pytest.raises(ValueError):
        Enhancer(norm='bogus')
