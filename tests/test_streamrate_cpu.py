"""CPU: the stream converter's contract.  tests/streamrate_ref.py - a history of K - 1 samples, D = half div down -
against resample_ref.resample of the whole signal, and the library's host functions (nele_resample_stream_delay / _hop_lengths /
_record_bytes / _state_bytes: no GPU call) against the formulas of the section.

Bound: 1e-13 of the output's peak (two float64 sums of K <= 385 products of the same operands in different orders: K eps64 = 8.5e-14
of sum |h x|, which stays below the peak here; measured at most 9.3e-16 for m >= D, 2.5e-17 for the first D outputs and 6.2e-16 for the flushed D)."""
import ctypes

import numpy as np
import pytest

import resample_ref as R
import streamrate_ref as S

HOPS = 4
CASES = [(a, b, q) for a, b in S.PAIRS for q in sorted(S.PRESETS)]


def _lib():
    import nele_gan_amd
    from nele_gan_amd import _lib, resample  # noqa: F401  (resample declares the signatures)
    return _lib


@pytest.mark.parametrize('sr_in,sr_out,quality', CASES)
def test_reference_is_the_offline_resampler_delayed_by_D(sr_in, sr_out, quality):
    up, down = S.ratio(sr_in, sr_out)
    zeros, beta = S.PRESETS[quality]
    n_in, n_out = S.hop_lengths(up, down, sr_out == S.RATE)
    h = R.taps(up, down, zeros, beta)
    ref = S.StreamRef(up, down, h, n_in)
    D = ref.D
    assert D == S.delay(up, down, zeros) and D <= n_out and ref.n_out == n_out
    x = np.random.RandomState(sr_in // 1000 + sr_out // 1000 + zeros).randn(HOPS * n_in)
    y = ref.run(x)
    assert y.shape == (HOPS * n_out,)
    whole = R.resample(x, up, down, h)
    assert len(whole) == HOPS * n_out
    peak = np.abs(whole).max()
    err = np.abs(y[D:] - whole[:len(whole) - D]).max()
    pre = np.abs(y[:D] - R.resample(x, up, down, h, outputs=range(-D, 0))).max()
    tail = np.abs(ref.flush() - whole[len(whole) - D:]).max()
    print('%d -> %d %s: D = %d, K = %d, m >= D %.2g, first D %.2g, flush %.2g of the peak; oldest read %d'
          % (sr_in, sr_out, quality, D, ref.K, err / peak, pre / peak, tail / peak, ref.oldest))
    assert err <= 1e-13 * peak and pre <= 1e-13 * peak and tail <= 1e-13 * peak
    assert np.abs(y[:D]).max() > 0.0                          # the first D outputs are the filter's pre-ringing, not zeros
    assert -(ref.K - 1) <= ref.oldest                          # no read outside history + hop (StreamRef.hop asserts the rest)
    assert not ref.hist.any()


def test_twelve_to_sixteen_has_a_phase_offset():
    """4 / 3 is the pair whose first output of a hop does not sit on phase 0: half - D down = 2"""
    up, down = S.ratio(12000, 16000)
    assert (up, down) == (4, 3)
    half = R.half_width(up, down, 32)
    assert S.delay(up, down, 32) == 42 and half - 42 * down == 2
    for a, b in S.PAIRS:
        if (a, b) != (12000, 16000):
            u, d = S.ratio(a, b)
            for z, _ in S.PRESETS.values():
                assert R.half_width(u, d, z) % d == 0


@pytest.mark.parametrize('sr_in,sr_out,quality', CASES)
def test_host_functions_match_the_formulas(sr_in, sr_out, quality):
    L = _lib()
    up, down = S.ratio(sr_in, sr_out)
    zeros, _ = S.PRESETS[quality]
    K = R.table_width(up, down, zeros)
    assert up * K * 8 <= 16384
    assert L.lib.nele_resample_stream_delay(up, down, zeros) == S.delay(up, down, zeros)
    n_in, n_out = ctypes.c_int(-7), ctypes.c_int(-7)
    assert L.lib.nele_resample_stream_hop_lengths(up, down, int(sr_out == S.RATE), ctypes.byref(n_in), ctypes.byref(n_out)) == 0
    assert (n_in.value, n_out.value) == S.hop_lengths(up, down, sr_out == S.RATE)
    assert n_in.value * up == n_out.value * down and S.HOP in (n_in.value, n_out.value)
    assert L.lib.nele_resample_stream_record_bytes(K) == S.record_bytes(K) >= 4 * (K - 1)
    for streams in (1, 3, 4096):
        assert L.lib.nele_resample_stream_state_bytes(streams, K) == S.state_bytes(streams, K)
    from nele_gan_amd.resample import stream_plan
    plan = stream_plan(sr_in, sr_out, quality)
    assert (plan['up'], plan['down'], plan['K'], plan['hop_in'], plan['hop_out'], plan['delay']) \
        == (up, down, K, n_in.value, n_out.value, S.delay(up, down, zeros))


def test_latencies_of_the_section():
    assert S.delay(1, 3, 32) == 32 and S.delay(1, 2, 32) == 32 and S.delay(2, 3, 32) == 32 and S.delay(1, 6, 32) == 32      # 2 ms at 16 kHz
    assert S.delay(1, 3, 10) == 10                            # 'scipy': 0.62 ms
    assert S.delay(2, 1, 32) == 64                            # 8 -> 16 kHz: 4 ms
    assert S.delay(3, 1, 32) == 96                            # 16 -> 48 kHz: 96 outputs at 48 kHz, 2 ms


def _refused(L, status, name):
    assert status == -1
    assert name.encode() in L.lib.nele_last_error_string()


def test_refusals_name_the_function_and_make_no_gpu_call():
    """44.1 kHz and its family, 16 001 Hz, zeros out of range, states that do not fit: -1 and the function's name, on a machine without a GPU"""
    L = _lib()
    n_in, n_out = ctypes.c_int(-7), ctypes.c_int(-7)
    for sr in (44100, 22050):
        up, down = S.ratio(sr, S.RATE)
        assert S.hop_lengths(up, down, True) is None
        _refused(L, L.lib.nele_resample_stream_hop_lengths(up, down, 1, ctypes.byref(n_in), ctypes.byref(n_out)), 'nele_resample_stream_hop_lengths')
        msg = L.lib.nele_last_error_string()
        assert b'44.1' in msg and b'nele_gan_amd.resample' in msg and (b'705.6' in msg or b'352.8' in msg)
        _refused(L, L.lib.nele_resample_stream_hop_lengths(down, up, 0, ctypes.byref(n_in), ctypes.byref(n_out)), 'nele_resample_stream_hop_lengths')
    up, down = S.ratio(16001, S.RATE)
    _refused(L, L.lib.nele_resample_stream_hop_lengths(up, down, 1, ctypes.byref(n_in), ctypes.byref(n_out)), 'nele_resample_stream_hop_lengths')
    _refused(L, L.lib.nele_resample_stream_delay(up, down, 32), 'nele_resample_stream_delay')
    assert (n_in.value, n_out.value) == (-7, -7)              # nothing written on a refusal
    _refused(L, L.lib.nele_resample_stream_hop_lengths(1, 3, 1, None, None), 'nele_resample_stream_hop_lengths')
    for zeros in (0, -1, 65):
        _refused(L, L.lib.nele_resample_stream_delay(1, 3, zeros), 'nele_resample_stream_delay')
    _refused(L, L.lib.nele_resample_stream_delay(1, 16, 64), 'nele_resample_stream_delay')      # K = 2049: a table above 16 KiB
    assert L.lib.nele_resample_stream_record_bytes(0) == -1 and L.lib.nele_resample_stream_record_bytes(2049) == -1
    assert L.lib.nele_resample_stream_state_bytes(0, 193) == -1 and L.lib.nele_resample_stream_state_bytes(4, 0) == -1
    # the launching entry points check their arguments before any GPU call: a 256-byte aligned host buffer stands in for the state
    raw = ctypes.create_string_buffer(4096 + 256)
    state = ctypes.c_void_p((ctypes.addressof(raw) + 255) // 256 * 256)
    for args in ((None, 4096, 1, 1, 3, 193), (state, 16, 1, 1, 3, 193), (state, 4096, 0, 1, 3, 193), (state, 4096, 1, 1, 3, 192),
                 (state, 4096, 1, 160, 441, 177)):
        _refused(L, L.lib.nele_resample_stream_init(*args, None), 'nele_resample_stream_init')
        _refused(L, L.lib.nele_resample_stream_reset(*args, None, None), 'nele_resample_stream_reset')
    ok = (state, 4096, 1, 1, 3, 193)
    buf = ctypes.c_void_p(ctypes.addressof(raw))
    for tail in ((None, buf, 768, None, 1, 768, buf, 256), (buf, None, 768, None, 1, 768, buf, 256), (buf, buf, 768, None, 0, 768, buf, 256),
                 (buf, buf, 768, None, 1, 767, buf, 256), (buf, buf, 767, None, 1, 768, buf, 256), (buf, buf, 768, None, 1, 768, buf, 255),
                 (buf, buf, 768, None, 1, 30, buf, 256)):       # the last: a hop of 10 outputs, shorter than the delay of 32
        _refused(L, L.lib.nele_resample_stream_hop(*ok, *tail, None), 'nele_resample_stream_hop')


def test_python_refuses_unsupported_rates_before_any_gpu_call():
    from nele_gan_amd.resample import StreamResampler, stream_plan
    for sr in (44100, 22050, 11025):
        with pytest.raises(ValueError, match='nele_gan_amd.resample'):
            stream_plan(sr, 16000)
        with pytest.raises(ValueError, match='44.1 kHz'):
            StreamResampler(3, 16000, sr)
    with pytest.raises(ValueError):
        stream_plan(16001, 16000)
    with pytest.raises(ValueError, match='16000'):
        stream_plan(8000, 48000)
    with pytest.raises(ValueError):
        stream_plan(48000, 16000, (0, 5.0))
    with pytest.raises(ValueError):
        StreamResampler(0, 48000, 16000)
