"""CPU: the numpy reference of the noise suppressor (tests/ns_ref.py, written from DESIGN.md section 21) on its own - its tracker
pinned to oracle.features.imcra_noise_psd bit for bit, the figures of section 21's table, a start on digital silence, the first 15
frames, a +10 dB noise step, E1 against scipy, and the all-flipped sensitivity experiment that tests/test_ns_gpu.py's bounds stand on
(tests/ns_cases.py holds every bound with its measured value)."""
import numpy as np
import pytest
import scipy.special

import ns_cases as K
from ns_ref import HOP, NBINS, ImcraTracker, NsRef, exp1


def test_the_tracker_with_the_cap_is_the_oracles_imcra_bit_for_bit():
    from oracle.features import imcra_noise_psd
    rng = np.random.default_rng(3)
    T = 160                                                                       # the minima ring wraps at frame 135
    a = (rng.standard_normal((NBINS, T)) * np.exp(rng.standard_normal((NBINS, T)))).astype(np.float32)
    a = (a.view(np.uint32) & np.uint32(0xFFFFF000)).view(np.float32)              # 11 mantissa bits: a * a is exact in float32
    Y = a.astype(np.complex64)                                                    # real-valued: np.abs(Y) ** 2 == a * a
    Y2 = np.abs(Y) ** 2
    assert Y2.dtype == np.float32 and np.array_equal(Y2.astype(np.float64), a.astype(np.float64) ** 2)
    want = imcra_noise_psd(Y)
    tr = ImcraTracker(p_cap=0.9)
    got = np.stack([np.asarray(tr.frame(Y2[:, l].copy())[3]).astype(np.float32) for l in range(T)], axis=1)
    assert np.isfinite(want).all() and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    free = ImcraTracker()                                                         # section 21's: the cap is the one deviation
    other = np.stack([np.asarray(free.frame(Y2[:, l].copy())[3]).astype(np.float32) for l in range(T)], axis=1)
    assert np.array_equal(other[:, :15], want[:, :15]) and not np.array_equal(other, want)


@pytest.mark.parametrize('kind,snr_db', K.SCENARIOS)
def test_figures_over_the_second_half(kind, snr_db):
    s, r = K.scenario(kind, snr_db), K.ref_run(kind, snr_db)
    att, lvl, before, after, split = K.figures(s['speech'], s['noise'], r['out'], r['gains'])
    print('%s %g dB: noise attenuated %.2f dB, speech level %.2f dB, error ratio %.3f -> %.3f, split %.2e' % (kind, snr_db, att, lvl, before, after, split))
    assert split <= K.MAX_SPLIT
    assert att >= K.MIN_NOISE_ATTENUATION_DB
    assert lvl >= K.MIN_SPEECH_LEVEL_CHANGE_DB
    assert after <= K.MAX_ERROR_RATIO_OF_INPUTS * before
    assert r['gains'].min() >= 0.1 * (1 - 1e-12) and r['gains'].max() <= 1.0 and 0.0 <= r['presence'].min() and r['presence'].max() <= 1.0


def test_a_start_on_digital_silence_stays_finite_and_silent():
    x = np.concatenate([np.zeros(40 * HOP, dtype=np.float32), K.scenario('pink', 10.0)['x'][:100 * HOP]])
    r = NsRef().run(x)
    for k in ('out', 'gains', 'noise_psd', 'presence'):
        assert np.isfinite(r[k]).all(), k
    assert not r['out'][:40 * HOP].any() and r['out'][41 * HOP:].any()
    assert (r['noise_psd'] > 0).all()


def test_the_first_fifteen_frames_come_out_at_gmin():
    s, r = K.scenario('pink', 10.0), K.ref_run('pink', 10.0)
    assert np.abs(r['gains'][:15] - 0.1).max() <= 4 * 2.0 ** -53 and np.abs(r['gains'][15] - 0.1).max() > 0.5
    assert not r['presence'][:15].any()
    one = NsRef(gmin=1.0).run(s['x'][:20 * HOP])
    assert np.abs(one['gains'][:15] - 1.0).max() <= 4 * 2.0 ** -53
    assert np.array_equal(one['out'][HOP:15 * HOP], s['x'][:14 * HOP])             # the input, one hop late
    assert np.abs(one['out'][:HOP]).max() <= 2.0 ** -40


def test_the_noise_estimate_follows_a_ten_db_step():
    n = K.STEP_HOPS_TOTAL * HOP
    v = K.noise('pink', n)
    v = 0.01 * v / np.sqrt(np.mean(v * v))
    v[K.STEP_HOP * HOP:] *= 10.0 ** (K.STEP_DB / 20.0)
    r = NsRef().run(v.astype(np.float32))
    level = np.mean(r['Y2f'][K.STEP_HOP + 2:].astype(np.float64))                 # the new level: the mean periodogram behind the step
    d = 10.0 * np.log10(r['noise_psd'].mean(axis=1) / level)
    inside = np.abs(d) <= K.STEP_WITHIN_DB
    first = int(np.argmax(inside[K.STEP_HOP:]))
    print('within %g dB %d hops after the step; the last 40 hops sit %.2f dB above the level; before the step %.2f dB above the old one'
          % (K.STEP_WITHIN_DB, first, d[-40:].mean(), d[K.STEP_HOP - 10:K.STEP_HOP].mean() + K.STEP_DB))
    assert inside[K.STEP_HOP + first] and first <= K.STEP_MAX_HOPS and inside[K.STEP_HOP + first:].all()
    assert abs(d[K.STEP_HOP - 10:K.STEP_HOP].mean() + K.STEP_DB) <= K.STEP_WITHIN_DB          # and it had the old level before


@pytest.mark.parametrize('kind,snr_db,hops', K.SENS_INPUTS)
def test_sensitivity_to_one_float32_ulp_of_every_power(kind, snr_db, hops):
    """the basis of the GPU bounds: measured again here, held under what ns_cases.py records (and not far under: the record is honest)"""
    s, base = K.scenario(kind, snr_db, hops), K.ref_run(kind, snr_db, hops)
    got = K.sensitivity(s['x'], base)
    print(kind, snr_db, hops, got)
    assert got['decisions'] == 0
    rec = K.SENS[(kind, snr_db, hops)]
    for k, v in rec.items():
        assert 0.8 * v <= got[k] <= v, (k, got[k], v)


def test_a_perturbation_below_float32_changes_nothing():
    s, base = K.scenario('pink', 10.0), K.ref_run('pink', 10.0)
    r = NsRef().run(s['x'].astype(np.float64) * (1.0 + 1e-15))
    assert np.array_equal(r['Y2f'], base['Y2f']) and np.array_equal(r['gains'], base['gains'])


def test_e1_against_scipy():
    x = np.concatenate([np.logspace(-8, 0, 20001)[:-1], np.logspace(0, np.log10(700.0), 20001), [1.0, np.nextafter(1.0, 0.0), 1.0000001]])
    rel = np.abs(exp1(x) / scipy.special.exp1(x) - 1.0).max()
    print('E1: largest relative deviation from scipy.special.exp1 over [1e-8, 700]: %.2e' % rel)
    assert rel <= 1e-13
    assert np.all(np.exp(0.5 * exp1(np.array([700.0, 1e3, 1e6, 1e300]))) == 1.0)  # beyond 700, exp(0.5 E1) is 1 to the last bit
