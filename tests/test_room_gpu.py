"""GPU: room.Room.apply - one RIR and one length per row - against oracle.evalpath.listening_condition row by row, and
eval_metrics.evaluate_rooms against the oracle's metric values.  Tolerances as in test_eval_gpu.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


def _rir(n=3000, seed=5, peak_at=37):
    rng = np.random.default_rng(seed)
    h = rng.standard_normal(n) * np.exp(-np.arange(n) / 400.0) * 0.2
    h[peak_at] = 1.0
    return h.astype(np.float32)


RIRS = {'MIRD_610': _rir(), 'AIR_stairway21': _rir(1700, 6, 5), 'hall': _rir(9001, 7, 120)}


def _peak_margin(v):
    """distance of a signal's extremes from clip()'s thresholds (max >= 1, min < -1)"""
    return min(abs(1.0 - np.max(v)), abs(-1.0 - np.min(v)))


def _oracle_stage_peaks(clean, enh, noise, rir, tau=32):
    """the three signals clip() sees in oracle.evalpath.listening_condition (restated to read the peaks; the comparison itself is
    against the oracle's own return values)"""
    from scipy.signal import lfilter
    from oracle import evalpath
    if rir is None:
        return [enh.astype(np.float64) + noise]
    b = int(np.argmax(rir))
    d = lfilter(np.hstack([rir[:b + tau], np.zeros(len(rir) - b - tau)]), [1], clean)
    r = lfilter(rir, [1], enh)
    d, r = d / evalpath.rms(d) * 0.03, r / evalpath.rms(r) * 0.03
    return [d, r, evalpath.clip(r)[b:] + noise[b:]]


def test_apply_matches_the_oracle_row_by_row():
    from nele_gan_amd import room, synth
    from oracle import evalpath
    assert torch.cuda.is_available()
    bank = room.RirBank(RIRS)
    c, v = synth.batch(5, 32000, start=70)
    enh = (c * np.float32(2.0)).copy()
    ids = np.asarray([0, 2, -1, 1, 1], np.int32)
    lens = np.asarray([31744, 20000, 32000, 25601, 31744], np.int32)
    v[4] *= np.float32(0.9 / np.abs(v[4]).max())                     # loud noise: row 4's last clip() divides (asserted below)
    v[4, 12345] = np.float32(1.2)
    for b in range(5):
        c[b, lens[b]:] = 0
        enh[b, lens[b]:] = 0
        v[b, lens[b]:] = 0
    clean_a, mixed, la = room.Room(bank).apply(torch.from_numpy(c).cuda(), torch.from_numpy(enh).cuda(), torch.from_numpy(v).cuda(), ids, lens)
    clean_a, mixed, la = clean_a.cpu().numpy(), mixed.cpu().numpy(), la.cpu().numpy()
    clipped = []
    for b in range(5):
        n = lens[b]
        rir = None if ids[b] < 0 else bank.rirs[ids[b]]
        ca, mx = evalpath.listening_condition(c[b, :n], enh[b, :n], v[b, :n], rir, enh_rms=0.0)
        # condition on the INPUTS: no peak within 1e-3 of clip()'s thresholds, so that rounding cannot change the number of divisions
        peaks = _oracle_stage_peaks(c[b, :n], enh[b, :n], v[b, :n], rir)
        for s in peaks:
            assert _peak_margin(s) >= 1e-3, (b, _peak_margin(s))
        clipped.append(any(np.max(s) >= 1 or np.min(s) < -1 for s in peaks))
        assert la[b] == len(ca) == len(mx) == n - (0 if rir is None else int(np.argmax(rir)))
        np.testing.assert_allclose(clean_a[b, :la[b]], ca, rtol=1e-5, atol=2e-8)
        np.testing.assert_allclose(mixed[b, :la[b]], mx, rtol=1e-5, atol=2e-8)
        assert not clean_a[b, la[b]:].any() and not mixed[b, la[b]:].any()
    assert clipped == [False, False, False, False, True]


def test_apply_with_enh_rms_and_default_lengths():
    from nele_gan_amd import room, synth
    from oracle import evalpath
    bank = room.RirBank(RIRS)
    c, v = synth.batch(2, 16384, start=90)
    enh = c * np.float32(3.0)
    ids = [1, -1]
    clean_a, mixed, la = room.Room(bank).apply(torch.from_numpy(c).cuda(), torch.from_numpy(enh).cuda(), torch.from_numpy(v).cuda(), ids, enh_rms=0.03)
    for b in range(2):
        rir = None if ids[b] < 0 else bank.rirs[ids[b]]
        ca, mx = evalpath.listening_condition(c[b], enh[b], v[b], rir, enh_rms=0.03)
        assert int(la[b]) == len(mx)
        np.testing.assert_allclose(clean_a[b, :len(ca)].cpu().numpy(), ca, rtol=1e-5, atol=2e-8)
        np.testing.assert_allclose(mixed[b, :len(mx)].cpu().numpy(), mx, rtol=1e-5, atol=2e-8)


def test_evaluate_rooms_raw_metrics_vs_oracle():
    from nele_gan_amd import eval_metrics, room, synth
    from oracle import evalpath, step
    bank = room.RirBank(RIRS)
    c, v = synth.batch(3, 32000, start=70)
    enh = (c * np.float32(2.0))[:, :31744]
    ids = np.asarray([0, -1, 1], np.int32)
    res = eval_metrics.evaluate_rooms(c, enh, v, bank, ids, metrics=('siib', 'estoi'))
    for b in range(3):
        rir = None if ids[b] < 0 else bank.rirs[ids[b]]
        ca, mx = evalpath.listening_condition(c[b], enh[b], v[b], rir)
        assert res['lengths'][b] == len(mx)
        ref = step.metric_targets(ca.astype(np.float32), mx.astype(np.float32), np.zeros(len(mx), np.float32), ['siib', 'estoi'], norm=False)
        assert res['siib'][b] == pytest.approx(ref[0], rel=2e-4, abs=1e-3)
        assert res['estoi'][b] == pytest.approx(ref[1], rel=2e-4, abs=2e-4)
    assert res['summary'].startswith('SIIB is ') and set(res['by_rir']) == {None, 'MIRD_610', 'AIR_stairway21'}
