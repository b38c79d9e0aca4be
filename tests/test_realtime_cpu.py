"""CPU: the real-time entry points (nele_rt_*) reject bad arguments without a GPU, their state-size arithmetic, and the host-side hop
bookkeeping of nele_gan_amd/realtime.py."""
import ctypes

import numpy as np
import pytest

LL = ctypes.c_longlong


def _lib():
    from nele_gan_amd import _lib
    return _lib.lib


def _err():
    return _lib().nele_last_error_string()


def test_state_bytes_grow_by_one_record_per_stream():
    lib = _lib()
    rec = lib.nele_rt_stream_record_bytes()
    assert rec > 0 and rec % 256 == 0
    base = lib.nele_rt_state_bytes(1) - rec
    assert base > 4 * 2093120                                       # at least one float32 copy of the generator's parameters
    for s in (1, 2, 16, 1024, 4096):
        assert lib.nele_rt_state_bytes(s) == base + s * rec
    assert lib.nele_rt_state_bytes(0) == -1
    assert lib.nele_rt_state_bytes(-3) == -1


def test_invalid_arguments_are_reported_with_their_names():
    lib = _lib()
    need = lib.nele_rt_state_bytes(4)
    fake = ctypes.c_void_p(1 << 20)                                 # never dereferenced: every call below fails its checks first
    cases = [
        (lambda: lib.nele_rt_init(None, LL(need), 4, fake, 0, None), b'nele_rt_init', b'state'),
        (lambda: lib.nele_rt_init(fake, LL(need - 1), 4, fake, 0, None), b'nele_rt_init', b'nele_rt_state_bytes'),
        (lambda: lib.nele_rt_init(fake, LL(need), 0, fake, 0, None), b'nele_rt_init', b'max_streams'),
        (lambda: lib.nele_rt_init(fake, LL(need), 4, None, 0, None), b'nele_rt_init', b'params_flat'),
        (lambda: lib.nele_rt_init(fake, LL(need), 4, fake, 2, None), b'nele_rt_init', b'precision'),
        (lambda: lib.nele_rt_set_weights(fake, LL(need), 4, None, 1, None), b'nele_rt_set_weights', b'params_flat'),
        (lambda: lib.nele_rt_reset(None, LL(need), 4, None, None), b'nele_rt_reset', b'state'),
        (lambda: lib.nele_rt_hop(fake, LL(need), 4, 0, None, fake, None, 1, None, fake, None, None, None, None, 0, None), b'nele_rt_hop', b'clean'),
        (lambda: lib.nele_rt_hop(fake, LL(need), 4, 0, fake, fake, None, 0, None, fake, None, None, None, None, 0, None), b'nele_rt_hop', b'nh'),
        (lambda: lib.nele_rt_hop(fake, LL(need), 4, 0, fake, fake, None, 1, None, fake, fake, None, None, None, 0, None), b'nele_rt_hop', b'dbg_frames'),
        (lambda: lib.nele_rt_hop(fake, LL(need), 4, 5, fake, fake, None, 1, None, fake, None, None, None, None, 0, None), b'nele_rt_hop', b'precision'),
        (lambda: lib.nele_rt_finish(fake, LL(need), 4, 0, fake, fake, None, None, fake, None, None, None, None, 0, None), b'nele_rt_finish', b'tail_lengths'),
        (lambda: lib.nele_rt_finish(fake, LL(need), 4, 0, fake, fake, fake, None, fake, None, None, None, None, -1, None), b'nele_rt_finish', b'dbg_frames'),
    ]
    for fn, name, what in cases:
        assert fn() == -1, (name, what)
        msg = _err()
        assert name in msg and what in msg, msg


def test_unaligned_state_is_rejected():
    lib = _lib()
    need = lib.nele_rt_state_bytes(2)
    assert lib.nele_rt_reset(ctypes.c_void_p((1 << 20) + 4), LL(need), 2, None, None) == -1
    assert b'aligned' in _err()


def test_host_hop_bookkeeping():
    from nele_gan_amd.realtime import advance
    hops = np.zeros(3, np.int64)
    emitted = np.zeros(3, np.int64)
    advance(hops, emitted, [True, True, False], 1)
    assert list(hops) == [1, 1, 0] and list(emitted) == [0, 0, 0]          # the first hop emits nothing
    advance(hops, emitted, [True, False, True], 1)
    assert list(hops) == [2, 1, 1] and list(emitted) == [256, 0, 0]
    advance(hops, emitted, [True, True, True], 7)
    assert list(hops) == [9, 8, 8] and list(emitted) == [256 * 8, 256 * 7, 256 * 7]
    # after n hops: 256 (n - 1) samples, whatever the grouping
    for groups in ([1] * 9, [3, 3, 3], [9], [2, 7]):
        h, e = np.zeros(1, np.int64), np.zeros(1, np.int64)
        for g in groups:
            advance(h, e, [True], g)
        assert h[0] == 9 and e[0] == 256 * 8


def test_enhancer_rejects_bad_settings_before_touching_a_device():
    from nele_gan_amd.realtime import RealtimeEnhancer
    with pytest.raises(ValueError, match='precision'):
        RealtimeEnhancer(streams=2, precision='fp8')
    with pytest.raises(ValueError, match='streams'):
        RealtimeEnhancer(streams=0, precision='f32')
