"""CPU: the carried high band on a hop schedule in float64 - tests/highband_sched_ref.py on schedrate_ref.SchedRef -
against the consequences the section states, the library's host plan against the reference's, and the refusals, which come before any
allocation.

Bounds.  Identity and the oracle identity: 0.0 - with enh = low delayed by lam the difference signal is an exact zero, and the shifted
converter's output m is the same K products in the same order as output m + a of the unshifted one fed b zeros first.  Low tones: 1e-5,
section 24's bound on what the added part may hold of the low band (the 'high' filters' ripple is near 1e-6 in amplitude); the same
measurement with s forced to 0 must exceed 1e-2 - a delay that is off by s / down of a sample leaves 2 sin(pi f s / (down rate)) of a
tone at f, 2.8e-2 at 1 kHz and 1.4e-1 at 5 kHz for the 0.2 samples of 44.1 kHz.  The tone at 0.75 x Nyquist: 1e-9, a thousand times
the 'high' stop band's 1e-12 in energy.
Measured here (the largest sample of the added part over the schedule's last period, which bounds the tone's amplitude from above):
identity 0.0 and oracle identity 0.0 in all cases; 1 kHz / 5 kHz at 44.1 kHz 2.45e-7 / 8.9e-7 (s = 0: 2.85e-2 / 1.42e-1; lag_hops 2,
where s = 0 is 0.6 samples off: 8.55e-2 / 4.24e-1), at 88.2 kHz 2.33e-7 / 8.86e-7, at 22.05 kHz 3.46e-7 / 8.31e-7; the 0.75 x Nyquist
tone: |a - g| <= 1.5e-14, quadrature <= 2.8e-14."""
from fractions import Fraction

import numpy as np
import pytest

import highband_ref as HB
import highband_sched_ref as HS
import resample_ref as R
import schedrate_ref as S

RATES = (22050, 44100, 88200)
# rate, preset, lag_hops -> section 20's latency, s, Lx, the shifted L0, E: the issue's table
TABLE = {(44100, 'high', 1): (Fraction(4414, 5), 32, 883, -160, 1), (44100, 'high', 2): (Fraction(7942, 5), 96, 1589, -224, 1),
         (22050, 'high', 1): (Fraction(4409, 10), 32, 441, 0, 1), (88200, 'high', 1): (Fraction(8823, 5), 32, 1765, -80, 1),
         (88200, 'high', 2): (Fraction(15879, 5), 16, 3176, -64, 1), (44100, 'scipy', 1): (Fraction(60893, 80), 134, 762, -204, 1),
         (22050, 'scipy', 1): (Fraction(60893, 160), 134, 381, -204, 2)}


@pytest.mark.parametrize('quality', ('high', 'scipy'))
@pytest.mark.parametrize('rate', RATES)
def test_the_librarys_plan_is_the_references_and_the_lag_a_whole_number(rate, quality):
    from nele_gan_amd import _lib
    from nele_gan_amd.highband import highband_sched_plan
    for lag_hops in (1, 2, 3):
        ref, got = HS.plan(rate, lag_hops, quality), highband_sched_plan(rate, lag_hops, quality)
        assert ref['exact'] and 0 <= ref['s'] < ref['down']
        assert (got['shift'], got['L0'], got['E'], got['H'], got['lag'], got['lag16']) == (ref['s'], ref['L0'], ref['E'], ref['H'], ref['Lx'], ref['lam'])
        assert (got['up'], got['down'], got['K'], got['delay'], got['delay_down']) == (ref['up'], ref['down'], ref['K'], ref['D_up'], ref['D_down'])
        assert Fraction(got['rnum'], got['period']) == ref['r'] and (got['hop_min'], got['hop_max']) == (int(ref['r']), -int(-ref['r'] // 1))
        assert 0 <= ref['Lx'] - ref['before'] < 1 and ref['Lx'] - ref['before'] == Fraction(ref['s'], ref['down'])
        assert _lib.lib.nele_hbsched_record_bytes(got['H'], got['lag16'], got['lag']) == HS.record_bytes(ref['H'], ref['lam'], ref['Lx'])
        assert _lib.lib.nele_hbsched_state_bytes(3, got['H'], got['lag16'], got['lag']) == HS.state_bytes(3, ref['H'], ref['lam'], ref['Lx'])
        if (rate, quality, lag_hops) in TABLE:
            assert (ref['before'], ref['s'], ref['Lx'], ref['L0'], ref['E']) == TABLE[(rate, quality, lag_hops)]
        a, b = HS.solve_ab(ref['up'], ref['down'], ref['s'])
        if (rate, quality, lag_hops) == (44100, 'high', 1):
            assert (a, b) == (88, 32)


def test_at_the_whole_hop_rates_the_plan_is_the_unscheduled_one():
    from nele_gan_amd.highband import highband_plan, highband_sched_plan
    for rate in (22000, 24000, 32000, 48000, 96000):
        for lag_hops in (1, 2):
            old, new = highband_plan(rate, lag_hops), highband_sched_plan(rate, lag_hops)
            assert new['shift'] == 0 and new['period'] == 1 and new['E'] == 0 and new['H'] == new['K'] - 1
            assert (new['lag'], new['lag16'], new['delay'], new['K'], new['hop_min']) == (old['lag'], old['lag16'], old['delay'], old['K'], old['hop_out'])
    odd = highband_sched_plan(22000, 1, 'scipy')                                 # D_down N / 256 = 13.75 samples: refused by section 24, shifted here
    ref = HS.plan(22000, 1, 'scipy')
    assert odd['shift'] == ref['s'] != 0 and odd['lag'] == ref['Lx'] == -int(-ref['before'] // 1)


@pytest.mark.parametrize('quality', ('high', 'scipy'))
@pytest.mark.parametrize('rate', RATES)
def test_every_assertion_of_the_schedule_holds_from_the_shifted_lead(rate, quality):
    """SchedRef.hop asserts on every hop: no read outside history + hop, L < down behind it, the swing W"""
    for lag_hops in (1, 2, 3):
        p = HS.plan(rate, lag_hops, quality)
        h = R.taps(p['up'], p['down'], p['zeros'], p['beta'])
        for pos in range(p['P']):
            c = HS.ShiftedSchedRef(p['up'], p['down'], h, p['s'], pos)
            assert (c.L0, c.E, c.H) == (p['L0'], p['E'], p['H'])
            d = np.random.RandomState(pos).randn((2 * p['P'] + 1) * S.HOP)
            y = c.run(d)
            assert min(c.leads) >= -c.E * c.up and c.oldest >= -c.H
            if lag_hops == 1 and pos in (0, p['P'] - 1):                         # hops and history change nothing: section 20's bound, 1e-13
                assert np.abs(y - HS.direct(d, p['up'], p['down'], h, p['L0'], len(y))).max() <= 1e-13 * np.abs(d).max()


@pytest.mark.parametrize('rate,lag_hops,groups', [(44100, 1, None), (44100, 2, (3, 4)), (22050, 1, (1, 2, 4)), (88200, 2, None)])
def test_an_enhancer_that_changes_nothing_gives_the_input_delayed_by_Lx(rate, lag_hops, groups):
    p = HS.plan(rate, lag_hops)
    x = np.random.RandomState(rate // 1000 + lag_hops).randn(S.widths(p['up'], p['down'], False, 0, 14)[1])
    y, plain, _ = HS.path(rate, x, HB.DelayedGain(p['lam'], 1.0), lag_hops, groups=groups)
    want = np.concatenate([np.zeros(p['Lx']), x])[:len(x)]
    err = float(np.abs(y - want).max())
    print('%d Hz, lag_hops %d: largest |y - x delayed by %d| = %g' % (rate, lag_hops, p['Lx'], err))
    assert err == 0.0
    assert np.abs(plain - want)[p['Lx']:].max() > 0.1                           # the plain wrapper is not the input


def _added_part(rate, f, lag_hops, quality, shift=None, g=1.0):
    """x[m - Lx] - up'(low delayed by lam)[m] for a unit tone at f over the last period of the schedule, and the delayed tone there"""
    p = HS.plan(rate, lag_hops, quality, shift)
    hops = (-(-10 // p['P']) + 1) * p['P']                                       # whole periods of the schedule; the last one starts at hop 10
    n = S.widths(p['up'], p['down'], False, 0, hops)[1]
    win = slice(n - S.widths(p['up'], p['down'], False, 0, p['P'])[1], n)
    m = np.arange(n)
    assert ((win.stop - win.start) * Fraction(f) / rate).denominator == 1        # whole periods of the tone
    y, _, hb = HS.path(rate, np.sin(2.0 * np.pi * f * m / rate), lambda low: np.zeros(len(low)), lag_hops, quality, g=g, shift=shift)
    assert hb.Lx == p['Lx']
    return y[win], np.sin(2.0 * np.pi * f * (m - p['Lx']) / rate)[win], np.cos(2.0 * np.pi * f * (m - p['Lx']) / rate)[win]


@pytest.mark.parametrize('rate,lag_hops', [(44100, 1), (44100, 2), (22050, 1), (88200, 1)])
def test_the_added_part_holds_none_of_a_low_tone_and_the_shift_is_why(rate, lag_hops):
    for f in (1000, 5000):
        amp = float(np.abs(_added_part(rate, f, lag_hops, 'high')[0]).max())
        off = float(np.abs(_added_part(rate, f, lag_hops, 'high', shift=0)[0]).max())
        print('%d Hz, lag_hops %d: of a unit %d Hz tone the added part holds %.3g; with s = 0 %.3g' % (rate, lag_hops, f, amp, off))
        assert amp < 1e-5
        assert off > 1e-2


@pytest.mark.parametrize('rate', (44100, 88200))
def test_a_tone_above_the_band_comes_out_at_the_gain(rate):
    for g in (1.0, 0.5):
        y, ref_s, ref_c = _added_part(rate, 0.375 * rate, 1, 'high', g=g)
        a, b = 2.0 * np.mean(y * ref_s), 2.0 * np.mean(y * ref_c)
        print('%d Hz, g %.1f: the %.1f Hz tone in phase g %+.3g, quadrature %.3g' % (rate, g, 0.375 * rate, a - g, b))
        assert abs(a - g) <= 1e-9 and abs(b) <= 1e-9


@pytest.mark.parametrize('rate,quality,lag_hops', [(44100, 'high', 1), (44100, 'high', 2), (22050, 'scipy', 1), (88200, 'high', 3)])
def test_the_shifted_converter_is_the_unshifted_one_b_zeros_and_a_outputs_on(rate, quality, lag_hops):
    """the oracle the GPU tests use: up'(d)[m] == up(b zeros + d)[m + a], a down - b up = -s"""
    p = HS.plan(rate, lag_hops, quality)
    h = R.taps(p['up'], p['down'], p['zeros'], p['beta'])
    a, b = HS.solve_ab(p['up'], p['down'], p['s'])
    for pos in (0, p['P'] - 1):
        nh = p['P'] + 2
        d = np.random.RandomState(7 + pos).randn(nh * S.HOP)
        got = HS.ShiftedSchedRef(p['up'], p['down'], h, p['s'], pos).run(d)
        pad = (-(-(b + len(d)) // S.HOP) + 2) * S.HOP - b - len(d)               # whole hops, two more than hold d: a < up outputs
        want = S.SchedRef(p['up'], p['down'], h, False, pos).run(np.concatenate([np.zeros(b), d, np.zeros(pad)]))
        assert len(want) >= len(got) + a
        err = float(np.abs(got - want[a:a + len(got)]).max())
        print('%d Hz %s, lag_hops %d, from %d: s = %d, a = %d, b = %d, largest difference %g' % (rate, quality, lag_hops, pos, p['s'], a, b, err))
        assert err == 0.0


def _no_gpu(monkeypatch):
    """a RealtimeEnhancer that never reached the GPU, and every allocation of a slot class an error"""
    import torch
    from nele_gan_amd import _slots
    from nele_gan_amd.realtime import RealtimeEnhancer

    def refuse(self, device, nbytes):
        raise AssertionError('reached the allocation of %s' % type(self).__name__)
    monkeypatch.setattr(_slots.SlotState, '_alloc', refuse)
    rt = object.__new__(RealtimeEnhancer)
    rt.S, rt.device = 2, torch.device('cpu')
    return rt


def test_refusals_come_before_any_allocation(monkeypatch):
    from nele_gan_amd.highband import ScheduledHighBandUp
    from nele_gan_amd.streamrate import FullBandScheduledEnhancer, RateAdaptedEnhancer, adapt_fullband
    rt = _no_gpu(monkeypatch)
    for rate in (8000, 11025, 16000):
        with pytest.raises(ValueError, match='no band'):
            ScheduledHighBandUp(2, rate)
    for rate in (8000, 11025):
        with pytest.raises(ValueError, match='no band'):
            FullBandScheduledEnhancer(rt, rate)
        with pytest.raises(ValueError, match='no band'):
            adapt_fullband(rt, rate)
    with pytest.raises(ValueError, match='lag_hops'):
        ScheduledHighBandUp(2, 44100, lag_hops=0)
    with pytest.raises(ValueError, match='lag_hops=9'):
        ScheduledHighBandUp(2, 44100, lag_hops=9)
    with pytest.raises(ValueError, match='streams'):
        ScheduledHighBandUp(0, 44100)
    with pytest.raises(ValueError, match='quality'):
        ScheduledHighBandUp(2, 44100, quality='best')
    for gain in (float('nan'), float('inf'), None):
        with pytest.raises(ValueError, match='finite'):
            FullBandScheduledEnhancer(rt, 44100, gain=gain)
    with pytest.raises(ValueError, match='finite'):
        adapt_fullband(rt, 44100, gain=float('nan'))
    with pytest.raises(ValueError, match='inner must be'):
        FullBandScheduledEnhancer(object(), 44100)
    # the checks passed: the next step is the first allocation
    with pytest.raises(AssertionError, match='reached the allocation of ScheduledHighBandUp'):
        ScheduledHighBandUp(2, 44100)
    for rate in (44100, 22050, 88200):
        with pytest.raises(AssertionError, match='reached the allocation of ScheduledStreamResampler'):
            FullBandScheduledEnhancer(rt, rate)
        with pytest.raises(AssertionError, match='reached the allocation of ScheduledStreamResampler'):
            adapt_fullband(rt, rate, gain=0.5)
    with pytest.raises(AssertionError, match='reached the allocation of ScheduledStreamResampler'):
        adapt_fullband(rt, 22000, quality='scipy')                               # 13.75 samples of delay: section 24 refuses, the shift serves
    with pytest.raises(AssertionError, match='reached the allocation of StreamResampler'):
        adapt_fullband(rt, 48000)                                                # where RateAdaptedEnhancer accepts the rate, it is that class
    # 16 kHz passes straight through
    for make in (FullBandScheduledEnhancer, adapt_fullband):
        same = make(rt, 16000)
        assert same.down is None and same.up is None and same.latency == 256
    assert type(adapt_fullband(rt, 16000)) is RateAdaptedEnhancer
