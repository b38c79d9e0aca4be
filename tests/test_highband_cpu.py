"""CPU: the carried high band's specification in float64 - tests/highband_ref.py on streamrate_ref.StreamRef -
against the consequences the section states, the geometry against the existing latency arithmetic, and the refusals, which come before
any GPU call.

Bounds.  Identity: 0.0 - with enh = low delayed by lam the difference signal is an exact zero.  Tone and both band energies: 1e-12 - the
stop band and the pass-band ripple of both 'high' filters are near 1e-6 in amplitude (-119 dB), 1e-12 in energy, and what the plain path
keeps of a stop-band tone passes both filters; in the high band the tones sit on the window's bins, so what the stop band lets through
lands on other bins and adds its energy, not its amplitude.
Measured here: identity 0.0 in all cases; 0.75 x Nyquist tone (10.5 kHz at 24 kHz) |a - g| <= 3.0e-13 with the band, <= 3.9e-13 left
by the plain wrapper; added part: <= 4.9e-13 of the input's energy below 6 kHz, 1 +- 2.8e-13 of it above 9.5 kHz (tones on the window's
bins: what the stop band lets through lands on other bins)."""
import numpy as np
import pytest

import highband_ref as HB
import streamrate_ref as S

RATES = (24000, 48000, 96000)
CASES = [(r, 1, None) for r in RATES] + [(48000, 1, (1, 2, 3, 1, 2, 3, 4)), (48000, 2, None), (24000, 2, (1, 2, 3, 1, 2, 3, 4)), (96000, 2, None)]
HOPS, FROM = 16, 12                                           # the window: the last 4 hops, a whole number of periods of every signal below


def _tone_hz(rate):
    return 10500.0 if rate == 24000 else 0.75 * rate / 2


@pytest.mark.parametrize('rate,lag_hops,groups', CASES)
def test_an_enhancer_that_changes_nothing_gives_the_input_delayed_by_L(rate, lag_hops, groups):
    geo = HB.geometry(rate, lag_hops)
    x = np.random.RandomState(rate // 1000 + lag_hops).randn(HOPS * geo['N'])
    y, plain = HB.path(rate, x, HB.DelayedGain(geo['lam'], 1.0), lag_hops, groups=groups)
    want = np.concatenate([np.zeros(geo['L']), x])[:len(x)]
    err = float(np.abs(y - want).max())
    print('%d Hz, lag_hops %d: largest |y - x delayed by %d| = %g' % (rate, lag_hops, geo['L'], err))
    assert err == 0.0
    assert np.abs(plain - want)[geo['L']:].max() > 0.1                          # the plain wrapper is not the input


@pytest.mark.parametrize('rate,lag_hops,groups', CASES)
def test_a_tone_above_the_band_comes_out_at_amplitude_one(rate, lag_hops, groups):
    geo = HB.geometry(rate, lag_hops)
    N, L, f = geo['N'], geo['L'], _tone_hz(rate)
    m = np.arange(HOPS * N)
    x = np.sin(2.0 * np.pi * f * m / rate)
    win = slice(FROM * N, HOPS * N)
    assert ((HOPS - FROM) * N * f / rate) % 1.0 == 0.0                          # whole periods
    ref_s, ref_c = np.sin(2.0 * np.pi * f * (m - L) / rate)[win], np.cos(2.0 * np.pi * f * (m - L) / rate)[win]
    for g in (1.0, 0.5):
        y, plain = HB.path(rate, x, HB.DelayedGain(geo['lam'], 2.0), lag_hops, g=g, groups=groups)
        a, b = 2.0 * np.mean(y[win] * ref_s), 2.0 * np.mean(y[win] * ref_c)
        left = np.hypot(2.0 * np.mean(plain[win] * ref_s), 2.0 * np.mean(plain[win] * ref_c))
        print('%d Hz, lag_hops %d, g %.1f: %.0f Hz tone in phase %.15f, quadrature %.3g; the plain wrapper leaves %.3g' % (rate, lag_hops, g, f, a, b, left))
        assert abs(a - g) <= 1e-12 and abs(b) <= 1e-12 and left <= 1e-12


def _band_signal(rate, N, lo_hz, hi_hz, seed):
    """unit tones with random phases on every multiple of 31.25 Hz in (lo_hz, hi_hz): periodic in two hops"""
    rs = np.random.RandomState(seed)
    m = np.arange(HOPS * N)
    x = np.zeros(len(m))
    for k in range(1, N):
        if lo_hz < k * 31.25 < hi_hz:
            x += np.sin(2.0 * np.pi * k * m / (2 * N) + rs.uniform(0.0, 2.0 * np.pi))
    return x / np.abs(x).max()


@pytest.mark.parametrize('rate,lag_hops,groups', CASES)
def test_the_added_part_holds_the_high_band_and_none_of_the_low(rate, lag_hops, groups):
    geo = HB.geometry(rate, lag_hops)
    N = geo['N']
    win = slice(FROM * N, HOPS * N)
    out = []
    for lo_hz, hi_hz in ((0.0, 6000.0), (9500.0, rate / 2.0)):
        x = _band_signal(rate, N, lo_hz, hi_hz, rate // 1000 + lag_hops)
        y, plain = HB.path(rate, x, HB.DelayedGain(geo['lam'], 2.0), lag_hops, groups=groups)
        added = (y - plain)[win]                                                 # x[m - L] - up(low delayed by lam)[m]
        out.append(float(np.sum(added ** 2) / np.sum(x[win] ** 2)))
    print('%d Hz, lag_hops %d: the added part holds %.3g of the energy below 6 kHz and 1 %+.3g of it above 9.5 kHz' % (rate, lag_hops, out[0], out[1] - 1.0))
    assert out[0] <= 1e-12
    assert abs(out[1] - 1.0) <= 1e-12


def test_fma32_is_the_correctly_rounded_float32_fma():
    """against exact rational arithmetic, on operands built to land on and beside float32 midpoints"""
    from fractions import Fraction
    rs = np.random.RandomState(5)
    a = rs.randn(400).astype(np.float32)
    b = rs.randn(400).astype(np.float32)
    c = rs.randn(400).astype(np.float32)
    a[:100], b[:100] = np.float32(1.0) + np.float32(2.0 ** -12) * rs.randint(1, 4096, 100).astype(np.float32), np.float32(1.0) + np.float32(2.0 ** -12)
    c[:100] = np.float32(2.0 ** -25) * rs.randint(-3, 4, 100).astype(np.float32)
    got = HB.fma32(a, b, c)
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        f = np.float32(float(exact))                                             # a candidate; the neighbours decide
        cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
        dist = [abs(Fraction(float(v)) - exact) for v in cands]
        best = min(dist)
        winners = [v for v, dd in zip(cands, dist) if dd == best]
        if len(winners) == 2:                                                    # a true tie: to even
            winners = [v for v in winners if (v.view(np.uint32) & 1) == 0]
        assert got[i] == winners[0], (i, a[i], b[i], c[i])


def test_the_lag_is_the_wrappers_latency_arithmetic():
    from nele_gan_amd.highband import highband_plan
    from nele_gan_amd.resample import stream_plan
    want = {22000: 440, 24000: 480, 32000: 640, 48000: 960, 64000: 1280, 96000: 1920}
    for rate in (22000, 24000, 32000, 48000, 64000, 96000):
        down, up = stream_plan(rate, S.RATE), stream_plan(S.RATE, rate)
        hop = down['hop_in']
        latency = down['delay'] * hop // S.HOP + hop + up['delay']              # RateAdaptedEnhancer._set_latency
        for lag_hops in (1, 2, 3):
            plan, geo = highband_plan(rate, lag_hops), HB.geometry(rate, lag_hops)
            assert plan['lag'] == geo['L'] == latency + (lag_hops - 1) * hop and plan['lag16'] == geo['lam'] == 256 * lag_hops
            assert (plan['up'], plan['down'], plan['hop_out'], plan['delay'], plan['delay_down']) == (geo['up'], geo['down'], geo['N'], geo['D_up'], geo['D_down'])
            assert (down['delay'] * hop) % S.HOP == 0
        assert latency == want[rate]


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


def test_refusals_come_before_any_gpu_call(monkeypatch):
    from nele_gan_amd.highband import HighBandUp, highband_plan
    from nele_gan_amd.streamrate import RateAdaptedEnhancer, ScheduledRateEnhancer, adapt
    rt = _no_gpu(monkeypatch)
    for rate in (8000, 12000, 16000):
        with pytest.raises(ValueError, match='no band'):
            HighBandUp(2, rate)
    for rate in (8000, 12000):
        with pytest.raises(ValueError, match='no band'):
            RateAdaptedEnhancer(rt, rate, highband=True)
        with pytest.raises(ValueError, match='no band'):
            adapt(rt, rate, highband=0.5)
    with pytest.raises(ValueError, match='13.75'):
        HighBandUp(2, 22000, quality='scipy')
    with pytest.raises(ValueError, match='not a whole number'):
        RateAdaptedEnhancer(rt, 22000, quality='scipy', highband=True)
    assert HB.geometry(22000, 1, 'scipy') is None and highband_plan(22000, 1, 'high')['lag'] == 440
    for rate in (44100, 22050):
        with pytest.raises(ValueError, match='fractional delay'):
            HighBandUp(2, rate)
        with pytest.raises(ValueError, match='fractional delay'):
            ScheduledRateEnhancer(rt, rate, highband=True)
        with pytest.raises(ValueError, match='fractional delay'):
            adapt(rt, rate, highband=True)
        with pytest.raises(ValueError, match='fractional delay'):
            RateAdaptedEnhancer(rt, rate, highband=True)
    with pytest.raises(ValueError, match='lag_hops'):
        HighBandUp(2, 48000, lag_hops=0)
    with pytest.raises(ValueError, match='lag_hops=9'):
        HighBandUp(2, 48000, lag_hops=9)
    with pytest.raises(ValueError, match='finite'):
        RateAdaptedEnhancer(rt, 48000, highband=float('nan'))
    with pytest.raises(ValueError, match='streams'):
        HighBandUp(0, 48000)
    # the checks passed: the next step is the first allocation
    with pytest.raises(AssertionError, match='reached the allocation of HighBandUp'):
        HighBandUp(2, 48000)
    with pytest.raises(AssertionError, match='reached the allocation of StreamResampler'):
        RateAdaptedEnhancer(rt, 48000, highband=True)
    # 16 kHz passes straight through, with or without the keyword
    for hb in (None, True):
        wrap = RateAdaptedEnhancer(rt, 16000, highband=hb)
        assert wrap.up is None and wrap.down is None and wrap.latency == 256


def test_lag_hops_follows_the_inner_object():
    from nele_gan_amd.aec import EchoCancellingEnhancer
    from nele_gan_amd.drc import CompressedEnhancer
    from nele_gan_amd.realtime import RealtimeEnhancer
    from nele_gan_amd.streamrate import RateAdaptedEnhancer

    def made(cls, **kw):
        obj = object.__new__(cls)
        obj.__dict__.update(kw)
        return obj
    rt = made(RealtimeEnhancer, S=2)
    comp = made(CompressedEnhancer, rt=rt, S=2)
    for inner, want in ((rt, 1), (made(EchoCancellingEnhancer, rt=rt, S=2), 1), (made(EchoCancellingEnhancer, rt=comp, S=2), 2)):
        assert made(RateAdaptedEnhancer, inner=inner)._lag_hops() == want
