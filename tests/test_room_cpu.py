"""CPU: the room entry points (csrc/fftconv.hip) are declared, exported and reject bad arguments without a GPU; RirBank's host side."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ('nele_rir_bank_bytes', 'nele_rir_bank_prepare', 'nele_fir_fft_workspace_bytes', 'nele_fir_fft_var', 'nele_norm_clip_var')


def test_header_declares_and_both_libraries_export_the_room_entry_points():
    from tests.test_capi_symbols import declared_symbols
    syms = declared_symbols()
    for lib in ('libnele_hip.so', 'libnele_hip_ab.so'):
        h = ctypes.CDLL(os.path.join(ROOT, 'nele_gan_amd', lib))
        for name in ENTRY:
            assert name in syms and hasattr(h, name), (lib, name)


def test_invalid_arguments_return_minus_one_and_name_the_entry_point():
    from nele_gan_amd import _lib, room  # noqa: F401  (room declares the signatures)
    lib = _lib.lib
    one = ctypes.c_void_p(256)                             # non-null, aligned, never dereferenced: every call below fails its checks first
    cases = [
        ('nele_rir_bank_bytes', lambda: lib.nele_rir_bank_bytes(0, 100)),
        ('nele_rir_bank_bytes', lambda: lib.nele_rir_bank_bytes(2, 0)),
        ('nele_fir_fft_workspace_bytes', lambda: lib.nele_fir_fft_workspace_bytes(0, 5)),
        ('nele_fir_fft_workspace_bytes', lambda: lib.nele_fir_fft_workspace_bytes(4, -1)),
        ('nele_rir_bank_prepare', lambda: lib.nele_rir_bank_prepare(None, one, 1, 10, one, None)),
        ('nele_rir_bank_prepare', lambda: lib.nele_rir_bank_prepare(one, one, 0, 10, one, None)),
        ('nele_rir_bank_prepare', lambda: lib.nele_rir_bank_prepare(one, one, 1, 10, ctypes.c_void_p(264), None)),
        ('nele_fir_fft_var', lambda: lib.nele_fir_fft_var(None, 1, 10, None, one, None, one, one, None)),
        ('nele_fir_fft_var', lambda: lib.nele_fir_fft_var(one, 0, 10, None, one, None, one, one, None)),
        ('nele_fir_fft_var', lambda: lib.nele_fir_fft_var(one, 1, 0, None, one, None, one, one, None)),
        ('nele_fir_fft_var', lambda: lib.nele_fir_fft_var(one, 1, 10, None, one, None, one, None, None)),
        ('nele_norm_clip_var', lambda: lib.nele_norm_clip_var(one, one, None, 1, 10, None, None, None, 0.0, one, None, None, None)),
        ('nele_norm_clip_var', lambda: lib.nele_norm_clip_var(one, None, None, 1, 0, None, None, None, 0.0, one, None, None, None)),
    ]
    for name, fn in cases:
        assert fn() == -1, name
        assert name.encode() in lib.nele_last_error_string(), (name, lib.nele_last_error_string())


def test_sizes_follow_the_block_count():
    from nele_gan_amd import _lib, room  # noqa: F401
    lib = _lib.lib
    assert lib.nele_fir_fft_workspace_bytes(256, 64000) == 256 * 250 * 4096
    assert lib.nele_fir_fft_workspace_bytes(1, 1) == 4096 and lib.nele_fir_fft_workspace_bytes(3, 257) == 3 * 2 * 4096
    assert lib.nele_rir_bank_bytes(2, 16000) >= 2 * 63 * 4096 and lib.nele_rir_bank_bytes(2, 16000) % 256 == 0


def _bank(**kw):
    from nele_gan_amd import room
    rng = np.random.default_rng(3)
    rirs = {}
    for k, (name, n, peak) in enumerate((('MIRD_610', 3000, 37), ('AIR_stairway21', 1700, 5), ('flat', 40, 0))):
        h = rng.standard_normal(n) * np.exp(-np.arange(n) / 400.0) * 0.2
        h[peak] = 1.0
        rirs[name] = h.astype(np.float32)
    return room.RirBank(rirs, **kw), rirs


def test_ids_follow_the_hash_convention():
    bank, _ = _bank()
    toy = sorted(f for f in os.listdir(os.path.join(ROOT, 'tests', 'golden', 'toy')) if f.endswith('.wav'))
    assert toy and (bank.ids(toy) == -1).all()                       # the toy files name no RIR
    names = ['spk1_003#MIRD_610#snr5.wav', '/corpus/Train/x#AIR_stairway21#0.wav', 'x#unknown#0.wav', 'plain.wav', 'a#flat.wav#b.wav']
    assert bank.ids(names).tolist() == [0, 1, -1, -1, 2]
    assert bank.ids(names).dtype == np.int32
    by_len, _ = _bank(resolver=lambda f: 'flat' if len(f) > 12 else None)
    assert by_len.ids(['short.wav', 'a_much_longer_name.wav']).tolist() == [-1, 2]
    assert bank.record()['names'] == ['MIRD_610', 'AIR_stairway21', 'flat'] and len(bank.record()['hash']) == 64


@pytest.mark.parametrize('tau', [32, 7])
def test_shift_and_direct_path_equal_the_oracles(tau):
    """oracle/evalpath.listening_condition: b = argmax(rir), h_direct = rir[:b + tau] followed by zeros"""
    from scipy.signal import lfilter
    bank, rirs = _bank(tau=tau)
    x = np.random.default_rng(1).standard_normal(500)
    for i, (name, h) in enumerate(rirs.items()):
        b = int(np.argmax(h))
        h_direct = np.hstack([h[:b + tau], np.zeros(len(h) - (b + tau))])
        assert bank.b[i] == b
        assert np.array_equal(bank.direct[i], h_direct[:b + tau]) and not h_direct[b + tau:].any()
        # (the trailing zeros filter nothing; scipy sums the two tap vectors in different orders, hence no bit equality)
        np.testing.assert_allclose(lfilter(bank.direct[i], [1], x), lfilter(h_direct, [1], x), rtol=0, atol=1e-13)
