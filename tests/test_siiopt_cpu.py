"""CPU: the float64 reference of the SII-optimal band gains (tests/siiopt_ref.py, written from DESIGN.md section 22) - that its
water-filling IS the optimum it claims, the figures of section 22's table with oracle.siib / oracle.estoi, and the sensitivity
experiment the GPU tolerance of tests/test_siiopt_gpu.py stands on."""
import numpy as np
import pytest

import siiopt_cases as S
import siiopt_ref as R


def _random_problem(rng):
    """(Sbar, N, gamma) spread over ten decades, some bands silent, some without importance"""
    Sbar = 10.0 ** rng.uniform(-10, 0, 64)
    N = 10.0 ** rng.uniform(-10, 0, 64)
    gamma = rng.uniform(0, 1, 64) ** 2
    Sbar[rng.uniform(size=64) < 0.05] = 0.0
    gamma[rng.uniform(size=64) < 0.1] = 0.0
    return Sbar, N, gamma / gamma.sum()


def _objective(p, N, gamma):
    return float(np.sum(gamma * p / (p + N)))


def test_water_filling_is_the_optimum_at_unchanged_power():
    rng = np.random.default_rng(11)
    better = tried = 0
    all_rounds = []
    for k in range(200):
        Sbar, N, gamma = _random_problem(rng)
        p = R.waterfill(Sbar, N, gamma, rounds=all_rounds)
        r = Sbar.sum()
        allowed = (gamma > 0) & (Sbar > 0)
        act = p > 0
        assert np.all(p >= 0) and not np.any(act & ~allowed)
        assert abs(p.sum() - r) <= 1e-12 * r
        # the Karush-Kuhn-Tucker conditions: the marginal gain gamma N / (p + N)^2 is equal over the active set and not larger on the
        # removed bands
        marg = gamma * N / (p + N) ** 2
        level = marg[act].mean()
        np.testing.assert_allclose(marg[act], level, rtol=1e-9)
        assert np.all(marg[allowed & ~act] <= level * (1 + 1e-9))
        # no random feasible perturbation scores higher: power moved between the allowed bands, rescaled to the same total
        f0 = _objective(p, N, gamma)
        for _ in range(50):
            q = p * np.exp(10.0 ** rng.uniform(-6, 0) * rng.standard_normal(64))
            q = q + (rng.uniform(size=64) < 0.1) * r * 10.0 ** rng.uniform(-8, -1)     # also into bands the solution removed
            q = np.where(allowed, q, 0.0)
            q *= r / q.sum()
            tried += 1
            better += _objective(q, N, gamma) > f0 * (1 + 1e-12)
    assert tried == 10000 and better == 0
    assert max(all_rounds) <= 64


def test_result_is_continuous_where_a_band_leaves_the_active_set():
    """a band removed at p = 0 leaves c unchanged: just below and just above the noise level at which a band leaves, every p agrees"""
    rng = np.random.default_rng(5)
    Sbar, N, gamma = _random_problem(rng)
    p = R.waterfill(Sbar, N, gamma)
    act = np.nonzero(p > 0)[0]
    i = act[np.argmin(p[act])]

    def at(Ni):
        N2 = N.copy()
        N2[i] = Ni
        return R.waterfill(Sbar, N2, gamma)
    lo, hi = N[i], N[i]
    while at(hi)[i] > 0:                                        # more noise in band i until the solution drops it
        hi *= 2
    for _ in range(200):                                        # the level at which it leaves, to the last bit
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        lo, hi = (mid, hi) if at(mid)[i] > 0 else (lo, mid)
    below, above = at(lo), at(hi)
    assert below[i] > 0 and above[i] == 0
    r = Sbar.sum()
    assert np.max(np.abs(below - above)) <= 1e-9 * r
    assert abs(below.sum() - r) <= 1e-12 * r and abs(above.sum() - r) <= 1e-12 * r


def test_default_importance_is_the_contracts_list():
    g = R.band_importance()
    assert g.shape == (64,) and abs(g.sum() - 1) < 1e-15 and np.all(g >= 0)
    assert np.all(g[31.25 * np.asarray(R.GMTBAND) < 160] == 0) and np.all(g[31.25 * np.asarray(R.GMTBAND) >= 160] > 0)
    # the density integrates back to the importances: bands between 1 and 4 kHz carry the sum of those one-third-octave bands (the band
    # edges do not coincide: a loose bound)
    f = 31.25 * np.asarray(R.GMTBAND, dtype=np.float64)
    mid = g[(f >= 900) & (f < 4500)].sum()
    assert 0.55 < mid < 0.75, mid                               # the list: 0.0818 + .. + 0.0771 = 0.6694 of 1 (before normalisation)
    from nele_gan_amd import siiopt
    np.testing.assert_allclose(siiopt.band_importance(), g, rtol=1e-14, atol=0)


@pytest.mark.parametrize('kind,snr', S.SCENARIOS)
def test_figures_of_the_table(kind, snr):
    s = S.scenario(kind, snr)
    b0, b1, e0, e1 = S.figures(s['speech'], s['noise'], S.ref_enhanced(kind, snr))
    print('%s %+.0f dB: raw SIIB %.2f -> %.2f (x %.3f), ESTOI %.4f -> %.4f' % (kind, snr, b0, b1, b1 / b0, e0, e1))
    assert b1 / b0 >= S.MIN_SIIB_RATIO[kind]
    assert e1 - e0 >= S.MIN_ESTOI_GAIN
    np.testing.assert_allclose((b0, b1, e0, e1), S.MEASURED[kind], rtol=2e-3)          # the values written beside the bounds are current
    enh = S.ref_enhanced(kind, snr)
    assert abs(np.sqrt(np.mean(enh ** 2)) - S.RMS) < 1e-12                            # unchanged power


def test_reversed_summation_order_moves_no_mask_value_by_an_eighth_of_the_gpu_bound():
    worst = 0.0
    for (kind, snr), (cb, nb) in zip(S.SCENARIOS, S.parity_inputs()):
        for strength in (0.5, 1.0):
            a = R.mask(cb, nb, strength=strength).astype(np.float64)
            b = R.mask(cb, nb, strength=strength, reverse=True).astype(np.float64)
            worst = max(worst, float(np.max(np.abs(a - b) / a)))
    print('largest relative deviation with reversed sums: %.3g' % worst)
    assert worst <= S.MAX_REVERSED_ORDER_DEVIATION


def test_edge_frames_of_the_reference_are_finite():
    """zero features (frames behind a row's end), NaN and zero noise, a silent start"""
    cb = np.zeros((6, 64), np.float32)
    nb = np.zeros((6, 64), np.float32)
    nb[1] = np.nan
    cb[3:] = S.features('white', 0.0)['cb'][50:53]
    nb[4] = S.features('white', 0.0)['nb'][50]
    m = R.mask(cb, nb)
    assert np.all(np.isfinite(m)) and np.all(m[:3] == 1.0)
    assert np.all((m >= np.float32(np.exp(-R.LOGMAX / 2)) * (1 - 1e-6)) & (m <= np.float32(np.exp(R.LOGMAX / 2)) * (1 + 1e-6)))
