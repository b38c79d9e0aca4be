"""CPU: the scheduled stream converter's contract.  tests/schedrate_ref.py - a history of K - 1 + E samples, a
lead, D = (half + W) div down - against resample_ref.resample of the whole signal from every starting position of the schedule, the
library's host functions (nele_sched_stream_plan / _widths / _record_bytes / _state_bytes: no GPU call) against the formulas and the
section's table, and the refusals of the C entry points and of the Python classes, all without a GPU.

Bound: 1e-13 of the output's peak, tests/test_streamrate_cpu.py's bound and reasoning (two float64 sums of K <= 385 products of the
same operands in different orders: K eps64 = 8.5e-14 of sum |h x|, which stays below the peak here).  Measured at most 9.1e-16 for
m >= D, 3.4e-17 for the first D outputs and 5.7e-16 for the flushed D, over all pairs, presets and starting positions."""
import ctypes

import numpy as np
import pytest

import resample_ref as R
import schedrate_ref as S
import streamrate_ref as S15

CASES = [(a, b, q) for a, b in S.PAIRS for q in sorted(S.PRESETS)]
# DESIGN.md section 20's table, 'high': (K, D, L0, E, H, lowest lead, highest lead over all starting positions)
TABLE = {(44100, 16000): (177, 32, 0, 1, 177, -128, 128), (22050, 16000): (89, 32, 0, 1, 89, -256, 256),
         (11025, 16000): (65, 47, -247, 2, 66, -759, 265), (88200, 16000): (353, 32, 0, 1, 353, -64, 64),
         (16000, 44100): (65, 89, -128, 1, 65, -256, 0), (16000, 22050): (65, 44, 32, 1, 65, -224, 288),
         (16000, 11025): (93, 32, 0, 2, 94, -512, 512)}
SCIPY_D = {(44100, 16000): 10, (22050, 16000): 10, (11025, 16000): 15, (88200, 16000): 10, (16000, 44100): 28, (16000, 22050): 14,
           (16000, 11025): 10}
SCHEDULES = {44100: [705, 706, 705, 706, 706], 22050: [352, 353, 353, 353, 353], 11025: [176, 176, 177, 176, 177],
             88200: [1411, 1411, 1411, 1411, 1412], 48000: [768], 12000: [192]}


def _lib():
    import nele_gan_amd
    from nele_gan_amd import _lib, resample  # noqa: F401
    return _lib


@pytest.mark.parametrize('sr_in,sr_out,quality', CASES)
def test_reference_is_the_offline_resampler_delayed_by_D_from_every_position(sr_in, sr_out, quality):
    up, down = S.ratio(sr_in, sr_out)
    zeros, beta = S.PRESETS[quality]
    to16k = sr_out == S.RATE
    h = R.taps(up, down, zeros, beta)
    p = S.plan(up, down, zeros, to16k)
    D, P = p['D'], p['P']
    assert D <= (S.HOP if to16k else p['hop_min'])
    worst, lo, hi = [0.0, 0.0, 0.0], p['L0'], p['L0']
    for g0 in range(P):
        ref = S.SchedRef(up, down, h, to16k, g0)
        n_in, T = S.widths(up, down, to16k, g0, 2 * P + 1)
        x = np.random.RandomState(sr_in // 1000 + sr_out // 1000 + zeros + g0).randn(n_in)
        y = ref.run(x)
        assert y.shape == (T,) and ref.pos == (g0 + 2 * P + 1) % P
        whole = R.resample(x, up, down, h, outputs=range(-D, T))          # y[m - D] for m in 0 .. T + D - 1
        peak = np.abs(whole).max()
        lo, hi = min(lo, min(ref.leads)), max(hi, max(ref.leads))
        assert -ref.H <= ref.oldest                               # no read outside history + hop (SchedRef.hop asserts the rest)
        tail = ref.flush()
        assert tail.shape == (D,) and not ref.hist.any() and ref.L == ref.L0
        worst = [max(worst[0], np.abs(y[D:] - whole[D:T]).max() / peak), max(worst[1], np.abs(y[:D] - whole[:D]).max() / peak),
                 max(worst[2], np.abs(tail - whole[T:]).max() / peak)]
        assert np.abs(y[:D]).max() > 0.0                          # the first D outputs are the filter's pre-ringing, not zeros
    print('%d -> %d %s: D = %d, K = %d, H = %d, leads %d .. %d; m >= D %.2g, first D %.2g, flush %.2g of the peak'
          % (sr_in, sr_out, quality, D, p['K'], p['H'], lo, hi, worst[0], worst[1], worst[2]))
    assert max(worst) <= 1e-13
    if quality == 'high' and (sr_in, sr_out) in TABLE:
        assert (lo, hi) == TABLE[(sr_in, sr_out)][5:]
    if P == 1:                                                    # section 15's plan
        assert (D, p['H'], p['E'], p['W']) == (S15.delay(up, down, zeros), p['K'] - 1, 0, 0)
        assert S.widths(up, down, to16k, 0, 1) == S15.hop_lengths(up, down, to16k)


def test_the_schedules_and_the_table_of_the_section():
    for sr, lengths in SCHEDULES.items():
        for to16k in (True, False):
            up, down = S.ratio(sr, S.RATE) if to16k else S.ratio(S.RATE, sr)
            got = [S.widths(up, down, to16k, g, 1)[0 if to16k else 1] for g in range(len(lengths))]
            assert got == lengths, (sr, to16k)
            assert S.plan(up, down, 32, to16k)['P'] == len(lengths)
    for (a, b), row in TABLE.items():
        up, down = S.ratio(a, b)
        p = S.plan(up, down, 32, b == S.RATE)
        assert (p['K'], p['D'], p['L0'], p['E'], p['H']) == row[:5], (a, b)
        assert S.plan(up, down, 10, b == S.RATE)['D'] == SCIPY_D[(a, b)]
        assert 220 * 1024 <= up * p['K'] * 8 <= 325 * 1024        # no table fits LDS
    assert S.record_bytes(177) == 768


@pytest.mark.parametrize('sr_in,sr_out,quality', CASES)
def test_host_functions_match_the_formulas(sr_in, sr_out, quality):
    L = _lib()
    up, down = S.ratio(sr_in, sr_out)
    zeros, _ = S.PRESETS[quality]
    to16k = int(sr_out == S.RATE)
    p = S.plan(up, down, zeros, to16k)
    info = (ctypes.c_int * L.CONSTS3['NELE_SCHED_INFO'])()
    assert L.lib.nele_sched_stream_plan(up, down, zeros, to16k, info) == 0
    assert list(info) == [p['K'], p['D'], p['L0'], p['E'], p['H'], p['r'].numerator, p['P'], p['hop_min'], p['hop_max']]
    for pos in range(p['P']):
        for nh in (1, 2, 3, p['P'], 2 * p['P'] + 1, 1000):
            n_in, n_out = ctypes.c_longlong(-7), ctypes.c_longlong(-7)
            assert L.lib.nele_sched_stream_widths(up, down, to16k, pos, nh, ctypes.byref(n_in), ctypes.byref(n_out)) == 0
            assert (n_in.value, n_out.value) == S.widths(up, down, to16k, pos, nh)
    assert L.lib.nele_sched_stream_record_bytes(p['H']) == S.record_bytes(p['H']) >= 16 + 4 * p['H']
    for streams in (1, 3, 4096):
        assert L.lib.nele_sched_stream_state_bytes(streams, p['H']) == S.state_bytes(streams, p['H'])
    from nele_gan_amd.resample import sched_plan
    got = sched_plan(sr_in, sr_out, quality)
    assert (got['up'], got['down'], got['K'], got['delay'], got['H'], got['period'], got['rnum']) \
        == (up, down, p['K'], p['D'], p['H'], p['P'], p['r'].numerator)


def _refused(L, status, name):
    assert status == -1
    assert name.encode() in L.lib.nele_last_error_string()


def test_refusals_name_the_function_and_make_no_gpu_call():
    L = _lib()
    info = (ctypes.c_int * L.CONSTS3['NELE_SCHED_INFO'])(*([-7] * L.CONSTS3['NELE_SCHED_INFO']))
    n_in, n_out = ctypes.c_longlong(-7), ctypes.c_longlong(-7)
    W = lambda *a: L.lib.nele_sched_stream_widths(*a, ctypes.byref(n_in), ctypes.byref(n_out))
    up, down = S.ratio(16001, S.RATE)
    _refused(L, L.lib.nele_sched_stream_plan(up, down, 32, 1, info), 'nele_sched_stream_plan')
    _refused(L, W(up, down, 1, 0, 1), 'nele_sched_stream_widths')
    for zeros in (0, -1, 65):
        _refused(L, L.lib.nele_sched_stream_plan(160, 441, zeros, 1, info), 'nele_sched_stream_plan')
    _refused(L, L.lib.nele_sched_stream_plan(160, 441, 32, 1, None), 'nele_sched_stream_plan')
    _refused(L, L.lib.nele_sched_stream_plan(1, 16, 32, 0, info), 'nele_sched_stream_plan')       # 16 -> 1 kHz: D = 32 outputs, hops of 16
    assert b'delay' in L.lib.nele_last_error_string()
    _refused(L, W(160, 441, 1, 5, 1), 'nele_sched_stream_widths')                                 # pos = P
    _refused(L, W(160, 441, 1, -1, 1), 'nele_sched_stream_widths')
    _refused(L, W(160, 441, 1, 0, 0), 'nele_sched_stream_widths')                                 # nh = 0
    _refused(L, L.lib.nele_sched_stream_widths(160, 441, 1, 0, 1, None, None), 'nele_sched_stream_widths')
    assert list(info) == [-7] * len(info) and (n_in.value, n_out.value) == (-7, -7)               # nothing written on a refusal
    assert L.lib.nele_sched_stream_record_bytes(-1) == -1 and L.lib.nele_sched_stream_record_bytes(4097) == -1
    assert L.lib.nele_sched_stream_state_bytes(0, 177) == -1 and L.lib.nele_sched_stream_state_bytes(4, -1) == -1
    # the launching entry points check their arguments before any GPU call: a 256-byte aligned host buffer stands in for the state
    raw = ctypes.create_string_buffer(8192 + 256)
    state = ctypes.c_void_p((ctypes.addressof(raw) + 255) // 256 * 256)
    need = S.state_bytes(1, 177)
    assert need == 1024
    for args in ((None, 4096, 1, 160, 441, 177, 1), (state, need - 1, 1, 160, 441, 177, 1), (state, 4096, 0, 160, 441, 177, 1),
                 (state, 4096, 1, 160, 441, 176, 1), (state, 4096, 1, 16000, 16001, 177, 1),
                 (ctypes.c_void_p(state.value + 16), 4096, 1, 160, 441, 177, 1)):
        _refused(L, L.lib.nele_sched_stream_init(*args, None), 'nele_sched_stream_init')
        _refused(L, L.lib.nele_sched_stream_reset(*args, None, None), 'nele_sched_stream_reset')
    ok = (state, 4096, 1, 160, 441, 177, 1)
    buf = ctypes.c_void_p(ctypes.addressof(raw))
    # (hp, x, x_stride, active, nh, pos, y, y_stride): from position 0 one hop is 705 -> 256, two are 1411 -> 512; from 1, 706 -> 256
    for tail in ((None, buf, 705, None, 1, 0, buf, 256), (buf, None, 705, None, 1, 0, buf, 256), (buf, buf, 705, None, 1, 0, None, 256),
                 (buf, buf, 705, None, 0, 0, buf, 256), (buf, buf, 705, None, 1, 5, buf, 256), (buf, buf, 705, None, 1, -1, buf, 256),
                 (buf, buf, 704, None, 1, 0, buf, 256), (buf, buf, 705, None, 1, 0, buf, 255), (buf, buf, 705, None, 1, 1, buf, 256),
                 (buf, buf, 1410, None, 2, 0, buf, 512), (buf, buf, 1411, None, 2, 0, buf, 511)):
        _refused(L, L.lib.nele_sched_stream_hop(*ok, *tail, None), 'nele_sched_stream_hop')
    away = (state, 4096, 1, 441, 160, 65, 0)                      # 16 -> 44.1 kHz: 256 -> 705 from position 0
    _refused(L, L.lib.nele_sched_stream_hop(*away, buf, buf, 256, None, 1, 0, buf, 704, None), 'nele_sched_stream_hop')
    _refused(L, L.lib.nele_sched_stream_hop(*away, buf, buf, 255, None, 1, 0, buf, 705, None), 'nele_sched_stream_hop')
    # 16 -> 1 kHz, zeros 32 (K = 1025): the delay of 32 outputs is longer than a hop of 16
    _refused(L, L.lib.nele_sched_stream_hop(state, 8192, 1, 1, 16, 1025, 0, buf, buf, 256, None, 1, 0, buf, 16, None), 'nele_sched_stream_hop')
    assert b'delay' in L.lib.nele_last_error_string()


class _NoGpu:
    """a ScheduledStreamResampler as far as its host bookkeeping goes: the checks under test come before the first GPU call"""

    def __new__(cls, streams, sr_in, sr_out, quality='high'):
        from nele_gan_amd.resample import ScheduledStreamResampler, sched_plan
        self = object.__new__(ScheduledStreamResampler)
        self.S = streams
        plan = sched_plan(sr_in, sr_out, quality)
        self.up, self.down, self.to16k, self.K, self.H = plan['up'], plan['down'], plan['to16k'], plan['K'], plan['H']
        self.delay, self.period, self._rnum = plan['delay'], plan['period'], plan['rnum']
        self.position, self.positions, self.hops = 0, np.zeros(streams, dtype=np.int64), np.zeros(streams, dtype=np.int64)
        self.device = 'no device'
        return self


def test_python_refuses_before_any_gpu_call():
    import torch
    from nele_gan_amd.resample import ScheduledStreamResampler, sched_plan
    from nele_gan_amd.streamrate import RateAdaptedEnhancer, ScheduledRateEnhancer, adapt
    with pytest.raises(ValueError):
        sched_plan(16001, 16000)
    with pytest.raises(ValueError, match='16000'):
        sched_plan(44100, 48000)
    with pytest.raises(ValueError):
        sched_plan(44100, 16000, (0, 5.0))
    with pytest.raises(ValueError, match='delay'):
        sched_plan(16000, 1000)
    with pytest.raises(ValueError):
        ScheduledStreamResampler(0, 44100, 16000)
    with pytest.raises(ValueError):
        ScheduledStreamResampler(2, 16001, 16000)
    sr = _NoGpu(3, 44100, 16000)
    assert [sr.width_in(1, g) for g in range(5)] == [705, 706, 705, 706, 706] and sr.width_out(3) == 768
    assert sr.width_in(5) == 3528 and sr.width_in(2, 4) == 706 + 705
    assert sr.call_plan(705) == (0, 1) and sr.call_plan(3528 + 705) == (0, 6)
    for width in (704, 706, 256, 1410, 1412):
        with pytest.raises(ValueError, match='width'):
            sr.process(torch.zeros((3, width)))
    with pytest.raises(ValueError, match='x must be'):
        sr.process(torch.zeros((4, 705)))
    with pytest.raises(ValueError, match='float32'):
        sr.process(torch.zeros((3, 705), dtype=torch.float64))
    with pytest.raises(ValueError, match='active'):
        sr.process(torch.zeros((3, 705)), active=[True] * 4)
    with pytest.raises(ValueError, match='position'):
        sr.width_in(1, 5)
    sr.positions[:] = [0, 0, 2]
    with pytest.raises(ValueError, match=r'slots \[2\]'):
        sr.process(torch.zeros((3, 705)))
    assert sr.call_plan(705, np.array([True, True, False])) == (0, 1)
    assert sr.call_plan(705, np.array([False, False, True])) == (2, 1)
    with pytest.raises(ValueError, match='width'):
        sr.call_plan(706, np.array([False, False, True]))
    assert sr.positions.tolist() == [0, 0, 2] and sr.position == 0 and not sr.hops.any()
    up = _NoGpu(2, 16000, 44100)
    assert [up.width_out(1, g) for g in range(5)] == [705, 706, 705, 706, 706] and up.width_in(3) == 768 and up.call_plan(512) == (0, 2)
    with pytest.raises(ValueError, match='width'):
        up.process(torch.zeros((2, 255)))
    for cls in (ScheduledRateEnhancer, RateAdaptedEnhancer):
        with pytest.raises(ValueError, match='%s: inner' % cls.__name__):
            cls(sr, 44100)
    with pytest.raises(ValueError, match='inner'):
        adapt(sr, 44100)
    with pytest.raises(ValueError, match='inner'):
        adapt(sr, 48000)
