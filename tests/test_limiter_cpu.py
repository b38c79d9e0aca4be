"""CPU: tests/limiter_ref.py - the float64 numpy restatement of DESIGN.md section 26 that the GPU limiter is held bit-equal to - against
an independent whole-signal form of the same contract, its streaming contract (hop grouping), the properties section 26 states, the
control of the peaks between the samples behind the 16 -> 48 kHz conversion, the figures of the limiter against turning the signal down
until it fits, and non-finite input.

Measured (tests/limiter_cases.py holds the figures the bounds stand on):
  property (a), g <= r: the mean of step 5 alone does not keep it in every bit - where the gain sits on r (a window of LA + 1 equal q)
  the rounding of the LA + 1 additions and of the division leaves the mean up to 13 ulps (2.0e-15 relative) above r at LA = 80, 37 ulps
  (5.1e-15) at LA = 192 and 1 ulp at LA = 1: on 12 of 15104 samples of the speech at +12 dB and on 18, 12 and 2 of the 2816 samples of
  the three tones.  Step 5 therefore ends with min(mean, r[n]); test_property_a_the_gain_never_exceeds_r holds g <= r exactly, and
  test_the_min_of_step_5_moves_the_gain_by_rounding_only holds the mean under r (1 + (LA + 3) 2^-53) at LA = 1, 80 and 192.
  property (b): (float) y exceeds cf on no sample of any input here before the clamp, and neither does (float)(mean s), the gain
  without step 5's min; with q = 1 before n = 0 (the start rule left out) (float)(mean s) of the tones at +6 dB exceeds it on 36, 26
  and 27 of their first 80 samples, the mean up to twice r.
"""
import numpy as np
import pytest

import limiter_cases as K
from limiter_ref import CEILING, HOP, RELEASE, LimRef, floor32, interpolated_max, reduction, taps

CF = floor32(CEILING)
PROPERTY_INPUTS = [('speech', o, 0, 60) for o in K.OVERS] + [('tone', f) for f in K.TONES]


def whole_signal(x, ceiling=CEILING, drive=1.0, lookahead=80, rel=RELEASE, true_peak=True, start_rule=True):
    """The contract on a whole signal at once, no hops and no state: LA zeros in front (the recursion's start), vectorised minima, the
    serial maximum, the first LA outputs dropped.  start_rule=False: the recursion starts at n = 0 and q = 1 before it (the variant the
    contract rejects).  -> dict: y, gain, mean (step 5's before its min), r, p [len(x)] float64; out float32"""
    LA, N = lookahead, len(x)
    lead = LA if start_rule else 0
    s = np.concatenate([np.zeros(lead), drive * x.astype(np.float64), np.zeros(LA)])           # s[n], n = -lead .. N + LA - 1
    z = np.concatenate([np.zeros(6), s, np.zeros(6)])
    p = np.abs(s)
    if true_peak:
        um = interpolated_max(z, taps())                                 # u[i], i = -lead - 1 .. N + LA - 1
        p = np.fmax(np.fmax(p, um[1:]), um[:-1])
    r = reduction(p, ceiling)
    n = lead + N
    m = r[:n].copy()
    for k in range(1, LA + 1):
        m = np.fmin(m, r[k:k + n])
    q = np.ones(LA + n)                                                  # q = 1 before the recursion's start
    d = 0.0
    for j in range(n):
        d = max(1.0 - m[j], rel * d)
        q[LA + j] = 1.0 - d
    acc = np.zeros(n)
    for k in range(LA + 1):
        acc = acc + q[k:k + n]
    mean = acc / float(LA + 1)
    g = np.fmin(mean, r[:n])
    y = g * s[:n]
    cf = floor32(ceiling)
    with np.errstate(over='ignore', invalid='ignore'):
        o = y.astype(np.float32)
    out = np.where(o > cf, cf, np.where(o < -cf, -cf, o)).astype(np.float32)
    return {'y': y[lead:], 'gain': g[lead:], 'mean': mean[lead:], 'r': r[lead:n], 'p': p[lead:n], 'out': out[lead:]}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def hop_peaks(p):
    return np.array([np.fmax.reduce(np.concatenate([[0.0], p[h * HOP:(h + 1) * HOP]])) for h in range(len(p) // HOP)])


# ------------------------------------------------------------------------------------------------ the two forms of the contract
@pytest.mark.parametrize('lookahead', [1, 80, 192])
@pytest.mark.parametrize('true_peak', [True, False])
@pytest.mark.parametrize('drive', [1.0, 4.0])
def test_the_streaming_reference_is_the_whole_signal_form_in_every_bit(lookahead, true_peak, drive):
    kw = dict(lookahead=lookahead, true_peak=true_peak, drive=drive)
    for key in (('speech', 12.0 if drive == 1.0 else 0.0, 0, 40), ('tone', 5333.0), ('burst',)):
        x = K.named(key)
        got, want = K.ref_run(key, **kw), whole_signal(x, **kw)
        n = len(x) - HOP
        assert not got['out'][:HOP].any() and not got['gain'][:HOP].any() and got['peak'][0] == 0
        for k in ('out', 'gain', 'mean', 'y', 'r'):
            assert same_bits(got[k][HOP:], want[k][:n]), (key, k)
        assert same_bits(got['peak'][1:], hop_peaks(want['p'][:n])), key
        assert got['gain'][HOP:].min() < 0.6                             # every one of them is limited


def test_every_hop_grouping_gives_the_same_bits_and_state():
    x = K.speech(12.0, shift=5000, hops=40)
    whole = LimRef()
    a = whole.run(x)
    for group in (1, 7):
        lim = LimRef()
        parts = [lim.run(x[i:i + group * HOP]) for i in range(0, len(x), group * HOP)]
        for k in a:
            assert same_bits(np.concatenate([p[k] for p in parts]), a[k]), (group, k)
        st, sw = lim.state(), whole.state()
        assert st['count'] == sw['count'] == 2 and st['d'] == sw['d'] and same_bits(st['hist'], sw['hist']) and same_bits(st['q'], sw['q'])
    assert whole.state()['q'].shape == (80,) and whole.state()['hist'].shape == (262,)


# ------------------------------------------------------------------------------------------------------------ the properties
@pytest.mark.parametrize('key', PROPERTY_INPUTS, ids=lambda k: '%s%+g' % (k[0], k[1]))
def test_property_a_the_gain_never_exceeds_r(key):
    """g <= r in every sample, as section 26 (a) states it"""
    r = K.ref_run(key)
    over = r['gain'][HOP:] > r['r'][HOP:]
    print('%s: g > r on %d samples, by %.3g relative at most' % (key, int(over.sum()), (r['gain'][HOP:][over] / r['r'][HOP:][over] - 1).max() if over.any() else 0))
    assert not over.any()


@pytest.mark.parametrize('lookahead', [1, 80, 192])
def test_the_min_of_step_5_moves_the_gain_by_rounding_only(lookahead):
    """Each of the LA + 1 additions, the division and the two subtractions of q = 1 - (1 - m) rounds once: the mean is at most
    r (1 + (LA + 3) u), u = 2^-53, to first order, so the min with r[n] takes back roundings and nothing else; it acts on some samples
    (the property would fail without it) and g is min(mean, r) in every bit."""
    acted = 0
    for key in PROPERTY_INPUTS:
        r = K.ref_run(key, lookahead=lookahead)
        g, rr, mean = r['gain'][HOP:], r['r'][HOP:], r['mean'][HOP:]
        assert np.all(mean <= rr * (1.0 + (lookahead + 3) * 2.0 ** -53)), key
        assert same_bits(g, np.fmin(mean, rr)) and np.all(g > 0) and np.all(g <= 1.0) and np.all(g <= rr)
        acted += int((mean > rr).sum())
    print('LA = %d: the mean is above r on %d samples of the %d inputs' % (lookahead, acted, len(PROPERTY_INPUTS)))
    assert acted > 0


@pytest.mark.parametrize('key', PROPERTY_INPUTS + [('burst',)], ids=lambda k: '%s%+g' % (k[0], k[1] if len(k) > 1 else 6))
def test_property_b_the_clamp_never_acts(key):
    """(float) y never exceeds cf before the clamp, with the gain and with the mean of step 5 before its min - on the tones the latter
    is the start rule's doing: their first sample is 6 dB over"""
    s = np.concatenate([np.zeros(HOP), K.named(key)[:-HOP].astype(np.float64)])           # drive 1, one hop late
    for kw in ({}, {'true_peak': False}, {'lookahead': 1}, {'lookahead': 192}):
        r = K.ref_run(key, **kw)
        o = r['y'].astype(np.float32)
        assert np.abs(o).max() <= CF and same_bits(o, r['out']), (key, kw)
        assert np.abs(r['out']).max() <= CF
        assert np.abs((r['mean'] * s).astype(np.float32)).max() <= CF, (key, kw)          # nor would it without step 5's min


def test_without_the_start_rule_an_abrupt_tone_is_cut_not_ramped():
    """q = 1 before n = 0 leaves the mean of a stream's first LA samples far above r: without step 5's min they would go to the clamp
    (a hard clip for 5 ms), with it the min does the clipping.  Either way the gain is no ramp; the bound of
    test_the_min_of_step_5_moves_the_gain_by_rounding_only is what tells the start rule from its absence."""
    bound = 1.0 + (80 + 3) * 2.0 ** -53
    for f in K.TONES:
        x = K.tone(f)
        bad, good = whole_signal(x, start_rule=False), whole_signal(x)
        over = np.nonzero(bad['mean'] > bad['r'] * bound)[0]
        clipped = int((np.abs((bad['mean'] * x.astype(np.float64)).astype(np.float32)) > CF).sum())
        print('%g Hz without the start rule: the mean is above r on %d samples, by x %.3f at most; (float)(mean s) is over cf on %d'
              % (f, len(over), (bad['mean'][over] / bad['r'][over]).max(), clipped))
        assert len(over) > 0 and over.max() < 80 and clipped > 0 and (bad['mean'][over] / bad['r'][over]).max() > 1.5
        assert np.all(good['mean'] <= good['r'] * bound) and not (np.abs((good['mean'] * x.astype(np.float64)).astype(np.float32)) > CF).any()


def test_property_c_below_the_ceiling_the_output_is_the_input_one_hop_late():
    for kw in ({}, {'true_peak': False}, {'lookahead': 1}, {'lookahead': 192}):
        key = ('speech', -3.0, 0, 60)
        x, r = K.named(key), K.ref_run(key, **kw)
        assert same_bits(r['out'][HOP:], x[:-HOP]) and np.all(r['gain'][HOP:] == 1.0) and r['peak'][1:].max() < CEILING
    # 4 kHz at 45 degrees, 1 dB over the ceiling: the samples are 3 dB under the crests between them - only the true-peak detector acts
    x = (CEILING * 10.0 ** (1.0 / 20.0) * np.cos(2.0 * np.pi * 0.25 * np.arange(12 * HOP) + np.pi / 4)).astype(np.float32)
    assert np.all(LimRef(true_peak=False).run(x)['gain'][HOP:] == 1.0) and LimRef().run(x)['gain'][HOP:].min() < 1.0


def test_the_gain_ramps_into_a_peak_and_releases():
    """one sample at twice the ceiling: the gain falls linearly over LA samples, is 1 / 2 at the peak, and is back within 1 % after
    five release times"""
    x = np.zeros(40 * HOP, np.float32)
    x[1000] = np.float32(2.0 * CEILING)
    g = LimRef(true_peak=False).run(x)['gain'][HOP:]
    assert np.all(g[:1000 - 80] == 1.0) and abs(g[1000] - 0.5) < 1e-7 and np.all(np.diff(g[1000 - 80:1001]) < 0)
    assert np.allclose(np.diff(g[1000 - 80:1001]), -0.5 / 81, rtol=1e-3, atol=0) and np.all(np.diff(g[1081:4000]) > 0)
    assert g[1000 + 80 + 8000] > 0.99


# -------------------------------------------------------------------------------------------------- between the samples
def test_the_taps_hold_the_peaks_between_the_samples():
    for name, x in K.true_peak_inputs().items():
        x1 = np.concatenate([x, np.zeros(HOP, np.float32)])
        with_taps, without = (K.peak_at_48k(LimRef(true_peak=tp).run(x1)['out']) for tp in (True, False))
        m = K.MEASURED_TRUE_PEAK[name]
        print('%s: peak at 48 kHz over the ceiling %.4f with the taps (measured %.4f), %.4f without (%.4f)' % (name, with_taps, m[0], without, m[1]))
        assert with_taps <= m[0] + K.TRUE_PEAK_ROOM and with_taps < without, name
        assert abs(with_taps - m[0]) < 5e-4 and abs(without - m[1]) < 5e-4, name          # MEASURED is current
    clipped = K.peak_at_48k(np.clip(K.speech(12.0), -CEILING, CEILING))
    print('a hard clip of the speech at +12 dB: %.4f' % clipped)
    assert clipped > 1.1


# ------------------------------------------------------------------------------------------------ against turning it down
@pytest.mark.parametrize('row', K.FIT_ROWS, ids=lambda r: '%s%+g_drive%+g' % r)
def test_the_limiter_against_scaled_to_fit(row):
    (siib_l, estoi_l), (siib_s, estoi_s) = K.fit_row(*row, how='limiter'), K.fit_row(*row, how='scaled')
    m = K.MEASURED[row]
    print('%s: raw SIIB %.2f against %.2f scaled to fit (x %.2f, measured x %.2f), ESTOI %.4f against %.4f'
          % (row, siib_l, siib_s, siib_l / siib_s, m[0] / m[1], estoi_l, estoi_s))
    assert siib_l / siib_s >= K.SIIB_MARGIN * (m[0] / m[1]) and estoi_l > estoi_s
    assert abs(siib_l / m[0] - 1) < 5e-3 and abs(siib_s / m[1] - 1) < 5e-3 and abs(estoi_l - m[2]) < 1e-3 and abs(estoi_s - m[3]) < 1e-3


# ------------------------------------------------------------------------------------------------------------- non-finite input
BAD_AT = 2914                                              # hop 11: two samples behind the speech's largest peak of its first 40 hops


def _with(value, over=12.0, hops=60):
    x = K.speech(over, hops=hops).copy()
    x[BAD_AT] = value
    return x


def test_a_nan_sample_leaves_through_the_output_and_not_into_the_state():
    """Section 26 (d): the NaN compares false in step 2 and is passed over by every max, so it asks for no reduction and the samples
    within 6 of it are judged by their own magnitude alone; the output is NaN in that one sample.  Against a run with a zero there,
    r differs within 6 samples of it, so d can differ until the next peak that sets it afresh: on this input every output, gain and
    state bit is the zero run's from hop 13 on (the sample is in hop 11, emitted in the call's hop 12, and 218 samples of that hop's
    gain differ)."""
    lim, zero = LimRef(), LimRef()
    a, z = lim.run(_with(np.nan)), zero.run(_with(0.0))
    assert np.array_equal(np.nonzero(np.isnan(a['out']))[0], [HOP + BAD_AT]) and np.isfinite(a['gain']).all() and np.isfinite(a['peak']).all()
    assert a['r'][HOP + BAD_AT] == 1.0
    near = slice(HOP + BAD_AT - 6, HOP + BAD_AT + 7)
    others = np.ones(len(a['r']), bool)
    others[near] = False
    assert same_bits(a['r'][others], z['r'][others]) and not same_bits(a['r'][near], z['r'][near])
    assert not same_bits(a['gain'][12 * HOP:13 * HOP], z['gain'][12 * HOP:13 * HOP])
    for k in ('out', 'gain', 'peak'):
        assert same_bits(a[k][13 * (HOP if k != 'peak' else 1):], z[k][13 * (HOP if k != 'peak' else 1):]), k
    sa, sz = lim.state(), zero.state()
    assert sa['d'] == sz['d'] and same_bits(sa['q'], sz['q']) and same_bits(sa['hist'], sz['hist']) and np.isfinite(sa['q']).all()


def test_an_infinite_sample_mutes_its_surroundings_and_is_released():
    """+inf: p is inf within 6 samples of it (each interpolator has one infinite term), r = c / inf = 0 there, the gain ramps to exactly
    0 over the look-ahead and y = 0 inf is NaN in that one sample; the state holds d = 1 and releases it at `rel` per sample.  The
    zero run's bits return with the first peak that asks for more reduction than what is left of it: from hop 17 on here."""
    lim, zero = LimRef(), LimRef()
    a, z = lim.run(_with(np.inf)), zero.run(_with(0.0))
    t = HOP + BAD_AT
    assert np.array_equal(np.nonzero(~np.isfinite(a['out']))[0], [t]) and np.isnan(a['out'][t])
    assert np.all(a['r'][t - 6:t + 7] == 0.0) and np.all(a['gain'][t - 6:t + 7] == 0.0) and not a['out'][t + 1:t + 7].any()
    assert np.all(np.diff(a['gain'][t - 6 - 80:t - 5]) < 0) and a['peak'][12] == np.inf
    assert np.isfinite(a['gain']).all() and np.abs(a['out'][np.isfinite(a['out'])]).max() <= CF
    first = 17
    assert not same_bits(a['gain'][(first - 1) * HOP:first * HOP], z['gain'][(first - 1) * HOP:first * HOP])
    for k in ('out', 'gain', 'peak'):
        assert same_bits(a[k][first * (HOP if k != 'peak' else 1):], z[k][first * (HOP if k != 'peak' else 1):]), k
    sa, sz = lim.state(), zero.state()
    assert sa['d'] == sz['d'] and same_bits(sa['q'], sz['q']) and same_bits(sa['hist'], sz['hist'])
