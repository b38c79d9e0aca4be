"""CPU: the bulk-delay search's C ABI (nele_bulk_* of include/nele_hip_ext.h: exported by both libraries, state-size arithmetic, bad
arguments rejected without a GPU; the header and the binding as a whole: tests/test_abi_ext_cpu.py), the numpy reference tests/bulk_ref.py on its own against
DESIGN.md section 16's lock hops, delays, negatives and end-to-end echo reductions, and AlignedEchoCanceller's bookkeeping on stubs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import aec_cases as C
import bulk_cases as BC
from aec_ref import AecRef
from bulk_ref import HOP, BulkRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LL = ctypes.c_longlong
ENTRY_POINTS = ('nele_bulk_state_bytes', 'nele_bulk_stream_record_bytes', 'nele_bulk_init', 'nele_bulk_reset', 'nele_bulk_set_delay',
                'nele_bulk_hop', 'nele_bulk_status')


def _lib():
    from nele_gan_amd import _lib
    return _lib.lib


def _err():
    return _lib().nele_last_error_string()


# ------------------------------------------------------------------------------------------------------------------------ the C ABI
def test_both_libraries_export_the_entry_points_and_the_product_reads_no_environment():
    for name in ('libnele_hip.so', 'libnele_hip_ab.so'):
        lib = ctypes.CDLL(os.path.join(ROOT, 'nele_gan_amd', name))
        assert [s for s in ENTRY_POINTS if not hasattr(lib, s)] == [], name
    nm = subprocess.run(['nm', '-D', '--undefined-only', os.path.join(ROOT, 'nele_gan_amd', 'libnele_hip.so')], stdout=subprocess.PIPE, text=True).stdout
    assert 'getenv' not in nm


def test_state_bytes_are_a_header_plus_one_record_per_stream():
    lib = _lib()
    for Q in (2, 3, 8, 32, 63, 64):
        rec = lib.nele_bulk_stream_record_bytes(Q)
        # the X ring and C (complex), the delay line (float32), S_d, S_x, x_prev, e
        assert rec >= 2 * Q * 257 * 16 - 2 * Q * 16 + Q * 1024 + 2 * 257 * 8 + 1024 + 8 * Q and rec % 256 == 0
        header = lib.nele_bulk_state_bytes(1, Q) - rec
        assert 0 < header <= 4096
        for B in (1, 2, 16, 1024, 4096):
            assert lib.nele_bulk_state_bytes(B, Q) == header + B * rec
    for B, Q in ((0, 8), (-1, 8), (4, 0), (4, 1), (4, 65), (4, -2), ((1 << 20) + 1, 8)):
        assert lib.nele_bulk_state_bytes(B, Q) == -1
    for Q in (0, 1, 65, -3):
        assert lib.nele_bulk_stream_record_bytes(Q) == -1


def test_bad_arguments_are_rejected_without_a_gpu():
    lib = _lib()
    B, Q = 4, 8
    need = lib.nele_bulk_state_bytes(B, Q)
    fake = ctypes.c_void_p(1 << 20)                                 # never dereferenced: every call below fails its checks first
    odd = ctypes.c_void_p((1 << 20) + 16)
    nan = float('nan')

    def hop(state=fake, nbytes=need, S=B, blocks=Q, mic=fake, played=fake, nh=1, lam=0.99, ratio=8.0, hold=16, aligned=fake):
        return lib.nele_bulk_hop(state, LL(nbytes), S, blocks, mic, played, None, nh, lam, ratio, hold, aligned, None, None)

    cases = [
        (lambda: hop(blocks=1, nbytes=1 << 40), b'nele_bulk_hop', b'blocks'),
        (lambda: hop(blocks=65, nbytes=1 << 40), b'nele_bulk_hop', b'blocks'),
        (lambda: hop(nh=0), b'nele_bulk_hop', b'nh'),
        (lambda: hop(mic=None), b'nele_bulk_hop', b'mic'),
        (lambda: hop(played=None), b'nele_bulk_hop', b'played'),
        (lambda: hop(aligned=None), b'nele_bulk_hop', b'null aligned'),
        (lambda: hop(state=None), b'nele_bulk_hop', b'state'),
        (lambda: hop(nbytes=need - 1), b'nele_bulk_hop', b'nele_bulk_state_bytes'),
        (lambda: hop(S=0), b'nele_bulk_hop', b'max_streams'),
        (lambda: hop(lam=0.0), b'nele_bulk_hop', b'lambda'),
        (lambda: hop(lam=1.0), b'nele_bulk_hop', b'lambda'),
        (lambda: hop(lam=nan), b'nele_bulk_hop', b'lambda'),
        (lambda: hop(ratio=1.0), b'nele_bulk_hop', b'ratio'),
        (lambda: hop(ratio=nan), b'nele_bulk_hop', b'ratio'),
        (lambda: hop(hold=0), b'nele_bulk_hop', b'hold'),
        (lambda: hop(state=odd), b'nele_bulk_hop', b'256-byte aligned'),
        (lambda: lib.nele_bulk_init(None, LL(need), B, Q, None), b'nele_bulk_init', b'state'),
        (lambda: lib.nele_bulk_init(fake, LL(need - 1), B, Q, None), b'nele_bulk_init', b'nele_bulk_state_bytes'),
        (lambda: lib.nele_bulk_init(fake, LL(1 << 40), B, 1, None), b'nele_bulk_init', b'blocks'),
        (lambda: lib.nele_bulk_init(fake, LL(1 << 40), B, 65, None), b'nele_bulk_init', b'blocks'),
        (lambda: lib.nele_bulk_init(fake, LL(need), 0, Q, None), b'nele_bulk_init', b'max_streams'),
        (lambda: lib.nele_bulk_init(odd, LL(need), B, Q, None), b'nele_bulk_init', b'256-byte aligned'),
        (lambda: lib.nele_bulk_reset(None, LL(need), B, Q, None, None), b'nele_bulk_reset', b'state'),
        (lambda: lib.nele_bulk_reset(fake, LL(need - 1), B, Q, None, None), b'nele_bulk_reset', b'nele_bulk_state_bytes'),
        (lambda: lib.nele_bulk_reset(fake, LL(1 << 40), B, 65, None, None), b'nele_bulk_reset', b'blocks'),
        (lambda: lib.nele_bulk_set_delay(None, LL(need), B, Q, None, fake, None), b'nele_bulk_set_delay', b'state'),
        (lambda: lib.nele_bulk_set_delay(fake, LL(need), B, Q, None, None, None), b'nele_bulk_set_delay', b'delay_hops'),
        (lambda: lib.nele_bulk_set_delay(fake, LL(need - 1), B, Q, None, fake, None), b'nele_bulk_set_delay', b'nele_bulk_state_bytes'),
        (lambda: lib.nele_bulk_set_delay(fake, LL(1 << 40), B, 1, None, fake, None), b'nele_bulk_set_delay', b'blocks'),
        (lambda: lib.nele_bulk_status(None, LL(need), B, Q, None, None, None, None, None), b'nele_bulk_status', b'state'),
        (lambda: lib.nele_bulk_status(fake, LL(need - 1), B, Q, None, None, None, None, None), b'nele_bulk_status', b'nele_bulk_state_bytes'),
        (lambda: lib.nele_bulk_status(fake, LL(need), 0, Q, None, None, None, None, None), b'nele_bulk_status', b'max_streams'),
        (lambda: lib.nele_bulk_status(odd, LL(need), B, Q, None, None, None, None, None), b'nele_bulk_status', b'256-byte aligned'),
    ]
    for i, (fn, name, what) in enumerate(cases):
        assert fn() == -1, (i, name, what)
        msg = _err()
        assert name in msg and what in msg, (i, msg)


def test_python_classes_reject_bad_settings_before_touching_a_device():
    from nele_gan_amd.bulkdelay import BulkDelay
    for kw, what in (({'streams': 0}, 'streams'), ({'blocks': 1}, 'blocks'), ({'blocks': 65}, 'blocks'), ({'lam': 0.0}, 'lam'), ({'lam': 1.0}, 'lam'),
                     ({'ratio': 1.0}, 'ratio'), ({'ratio': float('nan')}, 'ratio'), ({'hold': 0}, 'hold')):
        with pytest.raises(ValueError, match=what):
            BulkDelay(**dict({'streams': 2}, **kw))


# ---------------------------------------------------------------------------------------------------------------- the reference alone
_RUNS = {}


def ref_run(bulk, enr_db, seed):
    """(aligned, lock hop, BulkRef) at Q = 32 with the defaults: computed once, shared, never changed"""
    key = (bulk, enr_db, seed)
    if key not in _RUNS:
        s = BC.scenario(bulk, enr_db, seed)
        r = BulkRef(32)
        al, lock = r.run(s['mic'], s['played'])
        _RUNS[key] = (al, lock, r)
    return _RUNS[key]


@pytest.mark.parametrize('bulk,enr_db,seed,lock,delay', [(40, 10.0, 5, 46, 0), (1800, 0.0, 6, 46, 6), (1790, 0.0, 5, 112, 6), (5000, 0.0, 6, 72, 18),
                                                        (7000, 10.0, 5, 56, 26), (7900, 0.0, 6, 61, 30), (1800, -10.0, 5, 239, 6)])
def test_reference_locks_where_the_prototype_did(bulk, enr_db, seed, lock, delay):
    """the lock hop (0-based index of the first aligned hop) and the delay of DESIGN.md section 16's table; after alignment the main tap
    lies in 0 .. 767; aligned is zeros, then `played` late by the delay, bit for bit"""
    al, got_lock, r = ref_run(bulk, enr_db, seed)
    assert (got_lock, r.delay) == (lock, delay)
    assert 0 <= bulk - HOP * r.delay < 3 * HOP
    played = BC.scenario(bulk, enr_db, seed)['played']
    want = np.concatenate([np.zeros(HOP * delay, np.float32), played])[:len(played)]
    want[:lock * HOP] = 0.0
    assert np.array_equal(al, want) and al.dtype == np.float32
    assert r.n == lock + 1                                                       # no search work after the lock


def test_reference_does_not_lock_on_a_delay_beyond_the_range():
    al, lock, r = ref_run(9000, 10.0, 5)
    assert lock is None and r.delay == -1 and not al.any()
    assert max(l[3] for l in r.log) < 8.0


def test_reference_never_locks_without_an_echo():
    """white noise, the toy noise circularly shifted, the time-reversed far end circularly shifted (double talk), and played = 0"""
    worst = 0.0
    for name, mic, played in BC.negatives():
        r = BulkRef(32)
        al, lock = r.run(mic, played)
        assert lock is None and r.delay == -1 and not al.any(), name
        if played.any():
            worst = max(worst, max(l[3] for l in r.log))
        else:
            assert not r.e.any()                                                 # nothing played: every sum stays zero
    print('largest conf without an echo: %.2f (ratio 8)' % worst)
    assert worst < 8.0


def _reduction(echo, y, a=164, b=264):
    sl = slice(a * HOP, b * HOP)
    return 10.0 * np.log10(np.sum(echo[sl] ** 2) / np.sum((echo[sl] - y[sl]) ** 2))


def test_alignment_restores_the_cancellers_reduction():
    """echo reduction over hops 164 .. 263: `played` aligned by the found hops into P = 4 against the plain canceller at P = 8"""
    got = {}
    for bulk, enr_db, seed in ((40, 10.0, 5), (5000, 0.0, 6), (7000, 10.0, 5), (7900, 0.0, 6)):
        s = BC.scenario(bulk, enr_db, seed)
        _, y8 = AecRef(8).run(s['mic'], s['played'])
        _, y4 = AecRef(4).run(s['mic'], ref_run(bulk, enr_db, seed)[0])
        got[bulk] = (_reduction(s['echo'], y8), _reduction(s['echo'], y4))
        print('bulk %d: plain P = 8 %.1f dB, aligned P = 4 %.1f dB' % ((bulk,) + got[bulk]))
    for bulk in (5000, 7000, 7900):
        assert got[bulk][1] >= got[bulk][0] + 5.0, (bulk, got[bulk])
    assert abs(got[40][1] - got[40][0]) <= 2.0, got[40]


def test_set_delay_and_reset_in_the_reference():
    s = BC.scenario(1800, 0.0, 6, hops=12)
    r = BulkRef(4)
    r.set_delay(4)
    assert r.delay == -1                                                         # out of range: unchanged
    r.set_delay(2)
    al, lock = r.run(s['mic'], s['played'])
    assert lock == 0 and r.n == 0
    assert np.array_equal(al, np.concatenate([np.zeros(2 * HOP, np.float32), s['played']])[:len(al)])
    r.reset()
    assert r.delay == -1 and not r.line.any()


# ------------------------------------------------------------------------------------------------ AlignedEchoCanceller's bookkeeping
class _StubBulk:
    def __init__(self, S):
        self.S, self.calls, self.resets = S, [], []

    def process(self, mic, played, active=None, out=None):
        self.calls.append((mic.clone(), played.clone(), None if active is None else np.array(active, dtype=bool)))
        return 2.0 * played

    def reset(self, slots):
        self.resets.append(list(slots))


class _StubAec:
    def __init__(self, S):
        import torch
        self.S, self.P, self.device, self.calls, self.resets = S, 4, torch.device('cpu'), [], []

    def process(self, mic, played, active=None, adapt=None, want_echo=False, out=None):
        self.calls.append((mic.clone(), played.clone(), None if active is None else np.array(active, dtype=bool), adapt, want_echo, out))
        return (mic - played, played) if want_echo else mic - played

    def echo_path(self, slots=None):
        return ('path', slots)

    def reset(self, slots):
        self.resets.append(list(slots))


class _StubRt:
    def __init__(self, S):
        self.S, self.n, self.resets = S, 0, []

    def process(self, clean, noise, active=None):
        self.n += 1
        return clean + 0.5 * noise + float(self.n)

    def finish(self, slots, clean_tail, noise_tail, tail_lengths):
        return noise_tail

    def reset(self, slots):
        self.resets.append(list(slots))


def test_aligned_canceller_bookkeeping_on_stubs():
    import torch
    from nele_gan_amd.aec import EchoCancellingEnhancer
    from nele_gan_amd.bulkdelay import AlignedEchoCanceller
    S, W = 3, 2 * HOP
    bulk, aec, rt = _StubBulk(S), _StubAec(S), _StubRt(S)
    al = AlignedEchoCanceller(bulk, aec)
    assert (al.S, al.P, al.device) == (S, 4, aec.device)
    g = torch.Generator().manual_seed(5)
    mic, played = torch.rand(S, W, generator=g), torch.rand(S, W, generator=g)
    # process = aec.process(mic, bulk.process(mic, played, active), ...), every argument handed on
    res, echo = al.process(mic, played, active=[True, False, True], adapt=[True, True, False], want_echo=True, out='buffers')
    assert torch.equal(bulk.calls[0][0], mic) and torch.equal(bulk.calls[0][1], played) and list(bulk.calls[0][2]) == [True, False, True]
    m, p, act, adapt, want_echo, out = aec.calls[0]
    assert torch.equal(m, mic) and torch.equal(p, 2.0 * played) and list(act) == [True, False, True]
    assert adapt == [True, True, False] and want_echo is True and out == 'buffers'
    assert torch.equal(res, mic - 2.0 * played) and torch.equal(echo, 2.0 * played)
    assert torch.equal(al.process(mic, played), mic - 2.0 * played) and aec.calls[1][2:] == (None, None, False, None)
    assert al.echo_path([1]) == ('path', [1])
    al.reset([2, 0])
    assert bulk.resets == [[2, 0]] and aec.resets == [[2, 0]]
    with pytest.raises(ValueError, match='streams'):
        AlignedEchoCanceller(_StubBulk(2), _StubAec(3))
    # inside the closed loop: what the loop plays goes through the alignment, the loop's own bookkeeping is unchanged
    bulk, aec, rt = _StubBulk(S), _StubAec(S), _StubRt(S)
    loop = EchoCancellingEnhancer(rt, AlignedEchoCanceller(bulk, aec))
    clean = [torch.rand(S, W, generator=g) for _ in range(3)]
    mics = [torch.rand(S, W, generator=g) for _ in range(3)]
    out0 = loop.process(clean[0], mics[0])
    assert torch.equal(bulk.calls[0][1], torch.zeros(S, W)) and torch.equal(out0, clean[0] + 0.5 * mics[0] + 1.0)
    out1 = loop.process(clean[1], mics[1], active=[True, False, True])
    assert torch.equal(bulk.calls[1][1], out0) and list(bulk.calls[1][2]) == [True, False, True] and list(aec.calls[1][2]) == [True, False, True]
    assert torch.equal(aec.calls[1][1], 2.0 * out0)
    loop.process(clean[2], mics[2])
    assert torch.equal(bulk.calls[2][1][1], out0[1]) and torch.equal(bulk.calls[2][1][0], out1[0])
    loop.reset([1])
    assert rt.resets == [[1]] and bulk.resets == [[1]] and aec.resets == [[1]] and not loop.played[1].any()
    last = loop.finish([2], torch.rand(1, 100, generator=g), torch.rand(1, 100, generator=g), [100])
    assert last.shape == (1, HOP) and list(bulk.calls[-1][2]) == [False, False, True]
    with pytest.raises(ValueError, match='streams'):
        EchoCancellingEnhancer(_StubRt(2), AlignedEchoCanceller(_StubBulk(3), _StubAec(3)))
