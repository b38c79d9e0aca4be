"""CPU: the resampler's host side.  The library designs the filter on the host (nele_resample_taps: no HIP call), so
its taps, its polyphase table and its output lengths are checked here against scipy; tests/resample_ref.py - the closed form the GPU tests
compare the kernel with - is checked against scipy.signal.resample_poly; every refused argument is refused without a GPU; and the
loaders still raise on a file at another rate unless their switch is set.
Measured on the build this was written with: taps against up * firwin at most 1.33e-15 of the largest tap (640 / 441 'high', 40 961
taps; bound 1e-13); the restatement against resample_poly at most 8.7e-16 of the peak (bound 1e-13)."""
import ctypes
import os
import struct

import numpy as np
import pytest

import resample_ref as R


def _lib():
    from nele_gan_amd import _lib, resample  # noqa: F401  (resample declares the signatures)
    return _lib.lib


@pytest.mark.parametrize('preset', sorted(R.PRESETS))
@pytest.mark.parametrize('up,down', R.PAIRS)
def test_taps_against_firwin(up, down, preset):
    from nele_gan_amd import resample
    zeros, beta = R.PRESETS[preset]
    h = resample.taps(up, down, zeros, beta)
    want = R.scipy_taps(up, down, zeros, beta)
    assert h.shape == want.shape == (2 * zeros * max(up, down) + 1,)
    err = np.abs(h - want).max() / np.abs(want).max()
    print('taps %d/%d %s: %d taps, max |difference| %.3g of the largest tap' % (up, down, preset, len(h), err))
    assert err <= 1e-13
    assert np.abs(R.taps(up, down, zeros, beta) - want).max() / np.abs(want).max() <= 1e-13      # the restatement's own taps


@pytest.mark.parametrize('preset', sorted(R.PRESETS))
@pytest.mark.parametrize('up,down', R.PAIRS)
def test_polyphase_layout_bit_for_bit(up, down, preset):
    from nele_gan_amd import resample
    zeros, beta = R.PRESETS[preset]
    h = resample.taps(up, down, zeros, beta)
    hp = resample.taps(up, down, zeros, beta, layout=1)
    K = R.table_width(up, down, zeros)
    assert hp.shape == (up, K)
    want = R.polyphase(h, up)
    assert np.array_equal(hp.view(np.int64), want.view(np.int64))                # padding: +0.0 exactly
    for p in range(up):
        for k in (0, K - 1):
            j = p + k * up
            assert hp[p, k] == (h[j] if j < len(h) else 0.0)


@pytest.mark.parametrize('layout', (0, 1))
def test_taps_count_and_guard_words(layout):
    lib = _lib()
    for up, down in R.PAIRS:
        for zeros, beta in R.PRESETS.values():
            half = zeros * max(up, down)
            n = lib.nele_resample_taps_count(up, down, zeros, layout)
            assert n == (2 * half + 1 if layout == 0 else up * R.table_width(up, down, zeros))
            guard = 16
            buf = np.full(n + 2 * guard, -7.25)
            st = lib.nele_resample_taps(up, down, zeros, beta, layout, ctypes.c_void_p(buf.ctypes.data + 8 * guard))
            assert st == 0
            assert (buf[:guard] == -7.25).all() and (buf[-guard:] == -7.25).all()
            assert np.isfinite(buf[guard:-guard]).all() and (buf[guard:-guard] != -7.25).all()


def test_unit_ratio_is_the_unit_impulse():
    from nele_gan_amd import resample
    h = resample.taps(1, 1, 10, 5.0)
    assert h[10] == 1.0 and np.count_nonzero(h) == 1


@pytest.mark.parametrize('up,down', R.PAIRS)
def test_restatement_against_resample_poly(up, down):
    from nele_gan_amd import resample
    lib = _lib()
    assert lib.nele_resample_out_len(0, up, down) == 0 == R.out_len(0, up, down)
    rng = np.random.default_rng(up * 1000 + down)
    worst = 0.0
    for preset, (zeros, beta) in sorted(R.PRESETS.items()):
        h = resample.taps(up, down, zeros, beta)
        for L in (1, 2, 37, 700, 3001):
            x = rng.standard_normal(L)
            want = R.scipy_resample(x, up, down, h)
            assert lib.nele_resample_out_len(L, up, down) == len(want) == R.out_len(L, up, down)
            got = R.resample(x, up, down, h)
            worst = max(worst, np.abs(got - want).max() / np.abs(want).max())
    print('restatement against resample_poly %d/%d: at most %.3g of the peak' % (up, down, worst))
    assert worst <= 1e-13


def test_restatement_gain_and_selected_outputs():
    h = R.taps(3, 2, 10, 5.0)
    x = np.random.default_rng(5).standard_normal(100)
    y = R.resample(x, 3, 2, h)
    assert np.array_equal(R.resample(x, 3, 2, h, outputs=[0, 7, 149]), y[[0, 7, 149]])
    np.testing.assert_allclose(R.resample(x, 3, 2, h, gain=3.0), 3.0 * y, rtol=1e-15)


# ------------------------------------------------------------------------------------------------ refused arguments, no GPU
BAD_DESIGNS = (dict(up=0), dict(down=0), dict(up=1025, down=1024), dict(up=1024, down=1025), dict(up=1, down=17), dict(up=17, down=1),
               dict(up=-3), dict(zeros=0), dict(zeros=65), dict(beta=-0.5), dict(beta=20.5), dict(beta=float('nan')), dict(layout=2))


@pytest.mark.parametrize('bad', BAD_DESIGNS, ids=lambda b: ','.join('%s=%s' % kv for kv in b.items()))
def test_host_functions_refuse(bad):
    lib = _lib()
    a = dict(up=3, down=2, zeros=10, beta=5.0, layout=0)
    a.update(bad)
    buf = np.full(8, -7.25)                                  # never written: the checks come first
    assert lib.nele_resample_taps(a['up'], a['down'], a['zeros'], a['beta'], a['layout'], ctypes.c_void_p(buf.ctypes.data)) == -1
    assert b'nele_resample_taps' in lib.nele_last_error_string()
    assert (buf == -7.25).all()
    if 'beta' not in bad:
        assert lib.nele_resample_taps_count(a['up'], a['down'], a['zeros'], a['layout']) == -1
        assert b'nele_resample_taps_count' in lib.nele_last_error_string()
    if 'up' in bad or 'down' in bad:
        assert lib.nele_resample_out_len(100, a['up'], a['down']) == -1
        assert b'nele_resample_out_len' in lib.nele_last_error_string()


def test_host_functions_refuse_null_and_lengths():
    lib = _lib()
    assert lib.nele_resample_taps(3, 2, 10, 5.0, 0, None) == -1
    assert b'nele_resample_taps' in lib.nele_last_error_string()
    assert lib.nele_resample_out_len(-1, 3, 2) == -1 and lib.nele_resample_out_len((1 << 30) + 1, 3, 2) == -1
    assert b'nele_resample_out_len' in lib.nele_last_error_string()
    assert lib.nele_resample_out_len(1 << 30, 16, 1) == 16 << 30                                 # 64-bit


def _var(lib, **kw):
    """nele_resample_var with every pointer set to host memory that is never touched (the checks come first) unless overridden"""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    a = dict(x=p, x_stride=100, lengths_in=p, row_ids=None, R=1, Lmax_out=150, up=3, down=2, K=21, hp=p, gain=1.0, y=p, y_stride=150, lengths_out=p)
    a.update(kw)
    st = lib.nele_resample_var(a['x'], a['x_stride'], a['lengths_in'], a['row_ids'], a['R'], a['Lmax_out'], a['up'], a['down'], a['K'], a['hp'],
                               a['gain'], a['y'], a['y_stride'], a['lengths_out'], None)
    return st, lib.nele_last_error_string()


BAD_CALLS = (dict(up=0), dict(down=0), dict(up=1025, down=1024), dict(up=1024, down=1025), dict(up=1, down=17, K=21), dict(up=17, down=1, K=21),
             dict(K=0), dict(K=20), dict(K=2 * 65 + 1), dict(gain=float('inf')), dict(gain=float('nan')), dict(Lmax_out=0),
             dict(Lmax_out=(1 << 30) + 1, y_stride=(1 << 30) + 1), dict(R=0), dict(R=65536), dict(lengths_in=None), dict(x=None), dict(hp=None),
             dict(y=None), dict(lengths_out=None), dict(y_stride=149), dict(x_stride=0))


@pytest.mark.parametrize('bad', BAD_CALLS, ids=lambda b: ','.join('%s=%s' % kv for kv in b.items()))
def test_resample_var_refuses_without_a_gpu(bad):
    st, msg = _var(_lib(), **bad)
    assert st == -1 and b'nele_resample_var' in msg, (bad, st, msg)


def test_python_layer_refuses():
    import torch
    from nele_gan_amd import resample
    with pytest.raises(ValueError):
        resample.ratio(0, 16000)
    with pytest.raises(ValueError):
        resample.quality_params('best')
    with pytest.raises(ValueError):
        resample.taps(1, 17)
    with pytest.raises(ValueError):
        resample.out_len(-1, 1, 3)
    assert resample.ratio(44100, 16000) == (160, 441) and resample.ratio(8000, 16000) == (2, 1) and resample.ratio(16000, 16000) == (1, 1)
    assert resample.quality_params('high') == (32, 12.0) and resample.quality_params('scipy') == (10, 5.0) and resample.quality_params((7, 3)) == (7, 3.0)
    assert resample.out_len(13500000, 160, 441) == 4897960
    assert resample.TILE == _lib().nele_resample_tile() > 0
    with pytest.raises(ValueError):                          # a host tensor: there is no CPU path
        resample.resample(torch.zeros(1, 8), [8], 48000)


# ------------------------------------------------------------------------------------------------ the loaders' defaults are unchanged
def _write_wav(path, x, sr):
    body = np.clip(np.rint(np.asarray(x) * 32767.0), -32768, 32767).astype('<i2').tobytes()
    with open(path, 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', 36 + len(body)) + b'WAVEfmt ' + struct.pack('<IHHIIHH', 16, 1, 1, sr, sr * 2, 2, 16) + b'data'
                + struct.pack('<I', len(body)) + body)


def test_loaders_still_raise_without_the_switch(tmp_path):
    from nele_gan_amd import dataio, mixing, room
    p = str(tmp_path / 'n48.wav')
    _write_wav(p, 0.1 * np.sin(np.arange(480) * 0.1), 48000)
    with pytest.raises(ValueError, match='resampling on load is not part of the path'):
        dataio.load(p, sr=16000)
    x, sr = dataio.load(p)
    assert sr == 48000 and len(x) == 480
    with pytest.raises(ValueError, match='has sample rate 48000, expected 16000'):
        mixing.NoiseMixer([p], device='cpu')
    with pytest.raises(ValueError, match='48000 Hz, expected 16000'):
        room.RirBank(str(tmp_path), device='cpu')
    bank = room.RirBank({'a': np.asarray([0.0, 1.0, 0.5], dtype=np.float32)}, device='cpu')      # a dict never meets the rate check
    assert bank.names == ['a']


def test_command_line_arguments(tmp_path, capsys):
    from nele_gan_amd import resample
    empty = tmp_path / 'empty'
    empty.mkdir()
    for argv in (['--out', str(tmp_path)], ['--in', str(empty), '--out', str(tmp_path)], ['--in', str(empty), '--out', str(tmp_path), '--batch', '0'],
                 ['--in', str(empty), '--out', str(tmp_path), '--quality', 'best']):
        with pytest.raises(SystemExit) as e:
            resample.main(argv)
        assert e.value.code == 2
    capsys.readouterr()
