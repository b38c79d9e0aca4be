"""CPU: the delay tracker's C ABI (nele_track_* of include/nele_hip_ext.h: exported by both libraries, state-size arithmetic - the
bulk-delay search's, record for record - bad arguments rejected without a GPU; the header and the binding as a whole:
tests/test_abi_ext_cpu.py), the Python classes' refusals, the numpy reference
tests/track_ref.py on its own against DESIGN.md section 18's table (jumps followed, nothing moved without one), TrackedEchoCanceller's
bookkeeping on stubs, and the echo reduction of the reference chain behind a move with and without the canceller's restart."""
import ctypes
import os

import numpy as np
import pytest

import track_cases as TC
from aec_ref import AecRef
from bulk_ref import HOP, BulkRef
from track_ref import TrackRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LL = ctypes.c_longlong
ENTRY_POINTS = ('nele_track_state_bytes', 'nele_track_stream_record_bytes', 'nele_track_init', 'nele_track_reset', 'nele_track_set_delay',
                'nele_track_hop', 'nele_track_status')


def _lib():
    from nele_gan_amd import _lib
    return _lib.lib


def _err():
    return _lib().nele_last_error_string()


# ------------------------------------------------------------------------------------------------------------------------ the C ABI
def test_both_libraries_export_the_entry_points():
    for name in ('libnele_hip.so', 'libnele_hip_ab.so'):
        lib = ctypes.CDLL(os.path.join(ROOT, 'nele_gan_amd', name))
        assert [s for s in ENTRY_POINTS if not hasattr(lib, s)] == [], name


def test_state_bytes_are_a_header_plus_one_record_per_stream():
    lib = _lib()
    for Q in (2, 3, 8, 32, 64):
        rec = lib.nele_track_stream_record_bytes(Q)
        # the delay line (float32), the ring and C_q (complex128), e, x_prev, S_d, S_x; no more than 8 KB beside them
        need = Q * 256 * 4 + 2 * Q * 256 * 16 + Q * 8 + 256 * 4 + 2 * 257 * 8
        assert need <= rec <= need + 8192 and rec % 256 == 0, Q
        header = lib.nele_track_state_bytes(1, Q) - rec
        assert 0 < header <= 4096
        for B in (1, 2, 16, 4096, 1 << 20):
            assert lib.nele_track_state_bytes(B, Q) == header + B * rec
    for B, Q in ((0, 8), (-1, 8), ((1 << 20) + 1, 8), (4, 1), (4, 65), (4, 0)):
        assert lib.nele_track_state_bytes(B, Q) == -1
    for Q in (1, 65, -3):
        assert lib.nele_track_stream_record_bytes(Q) == -1


def test_the_tracker_and_the_plain_search_share_one_record_layout():
    """one layout for both sets of entry points: the sizes are what each has always returned, 6144 + 9216 Q bytes a record"""
    lib = _lib()
    for Q in range(2, 65):
        assert lib.nele_track_stream_record_bytes(Q) == lib.nele_bulk_stream_record_bytes(Q) == 6144 + 9216 * Q
        for B in (1, 3, 1 << 20):
            assert lib.nele_track_state_bytes(B, Q) == lib.nele_bulk_state_bytes(B, Q) == 256 + B * (6144 + 9216 * Q)


def test_bad_arguments_are_rejected_without_a_gpu():
    lib = _lib()
    B, Q = 4, 8
    need = lib.nele_track_state_bytes(B, Q)
    fake = ctypes.c_void_p(1 << 20)                                 # never dereferenced: every call below fails its checks first
    odd = ctypes.c_void_p((1 << 20) + 16)
    nan, inf = float('nan'), float('inf')

    def hop(state=fake, nbytes=need, S=B, blocks=Q, mic=fake, played=fake, nh=1, lam=0.99, ratio=8.0, hold=16, patience=128, rest=0, aligned=fake):
        return lib.nele_track_hop(state, LL(nbytes), S, blocks, mic, played, None, nh, lam, ratio, hold, patience, rest, aligned, None, None)

    cases = [
        (lambda: hop(state=None), b'nele_track_hop', b'state'),
        (lambda: hop(nbytes=need - 1), b'nele_track_hop', b'nele_track_state_bytes'),
        (lambda: hop(S=0), b'nele_track_hop', b'max_streams'),
        (lambda: hop(S=(1 << 20) + 1, nbytes=1 << 50), b'nele_track_hop', b'max_streams'),
        (lambda: hop(blocks=1), b'nele_track_hop', b'blocks'),
        (lambda: hop(blocks=65, nbytes=1 << 40), b'nele_track_hop', b'blocks'),
        (lambda: hop(state=odd), b'nele_track_hop', b'256-byte aligned'),
        (lambda: hop(mic=None), b'nele_track_hop', b'mic'),
        (lambda: hop(played=None), b'nele_track_hop', b'played'),
        (lambda: hop(aligned=None), b'nele_track_hop', b'aligned'),
        (lambda: hop(nh=0), b'nele_track_hop', b'nh'),
        (lambda: hop(nh=(1 << 20) + 1), b'nele_track_hop', b'nh'),
        (lambda: hop(lam=0.0), b'nele_track_hop', b'lambda'),
        (lambda: hop(lam=1.0), b'nele_track_hop', b'lambda'),
        (lambda: hop(lam=nan), b'nele_track_hop', b'lambda'),
        (lambda: hop(ratio=1.0), b'nele_track_hop', b'ratio'),
        (lambda: hop(ratio=inf), b'nele_track_hop', b'ratio'),
        (lambda: hop(ratio=nan), b'nele_track_hop', b'ratio'),
        (lambda: hop(hold=0), b'nele_track_hop', b'hold'),
        (lambda: hop(patience=0), b'nele_track_hop', b'patience'),
        (lambda: hop(patience=-5), b'nele_track_hop', b'patience'),
        (lambda: hop(rest=-1), b'nele_track_hop', b'rest'),
        (lambda: lib.nele_track_init(None, LL(need), B, Q, None), b'nele_track_init', b'state'),
        (lambda: lib.nele_track_init(fake, LL(need - 1), B, Q, None), b'nele_track_init', b'nele_track_state_bytes'),
        (lambda: lib.nele_track_init(fake, LL(need), 0, Q, None), b'nele_track_init', b'max_streams'),
        (lambda: lib.nele_track_init(fake, LL(need), B, 1, None), b'nele_track_init', b'blocks'),
        (lambda: lib.nele_track_init(odd, LL(need), B, Q, None), b'nele_track_init', b'256-byte aligned'),
        (lambda: lib.nele_track_reset(None, LL(need), B, Q, None, None), b'nele_track_reset', b'state'),
        (lambda: lib.nele_track_reset(fake, LL(need - 1), B, Q, None, None), b'nele_track_reset', b'nele_track_state_bytes'),
        (lambda: lib.nele_track_reset(fake, LL(need), -3, Q, None, None), b'nele_track_reset', b'max_streams'),
        (lambda: lib.nele_track_reset(odd, LL(need), B, Q, None, None), b'nele_track_reset', b'256-byte aligned'),
        (lambda: lib.nele_track_set_delay(None, LL(need), B, Q, None, fake, None), b'nele_track_set_delay', b'state'),
        (lambda: lib.nele_track_set_delay(fake, LL(need), B, Q, None, None, None), b'nele_track_set_delay', b'delay_hops'),
        (lambda: lib.nele_track_set_delay(fake, LL(need), B, 65, None, fake, None), b'nele_track_set_delay', b'blocks'),
        (lambda: lib.nele_track_status(None, LL(need), B, Q, None, None, None, None), b'nele_track_status', b'state'),
        (lambda: lib.nele_track_status(fake, LL(need - 1), B, Q, None, None, None, None), b'nele_track_status', b'nele_track_state_bytes'),
        (lambda: lib.nele_track_status(odd, LL(need), B, Q, None, None, None, None), b'nele_track_status', b'256-byte aligned'),
    ]
    for i, (fn, name, what) in enumerate(cases):
        assert fn() == -1, (i, name, what)
        msg = _err()
        assert name in msg and what in msg, (i, msg)


def test_python_classes_reject_bad_settings_before_touching_a_device():
    from nele_gan_amd.bulktrack import TrackedEchoCanceller, TrackingBulkDelay
    nan = float('nan')
    for kw, what in (({'streams': 0}, 'streams'), ({'blocks': 1}, 'blocks'), ({'blocks': 65}, 'blocks'), ({'lam': 1.0}, 'lam'), ({'lam': nan}, 'lam'),
                     ({'ratio': 1.0}, 'ratio'), ({'ratio': float('inf')}, 'ratio'), ({'hold': 0}, 'hold'), ({'patience': 0}, 'patience'),
                     ({'rest': -1}, 'rest')):
        with pytest.raises(ValueError, match=what):
            TrackingBulkDelay(**dict({'streams': 2}, **kw))
    with pytest.raises(ValueError, match='streams'):
        TrackedEchoCanceller(_StubTrack(2), _StubAec(3))


# ---------------------------------------------------------------------------------------------------------------- the reference alone
HOPS, JUMP, Q = 792, 264, 32
JUMPS = ((40, 3000), (2000, 5000), (7000, 1000), (3000, 300))
_RUNS = {}


def _run(bulk_a, bulk_b, enr_db, seed, jump=JUMP, mute=None):
    key = (bulk_a, bulk_b, enr_db, seed, jump, mute)
    if key not in _RUNS:
        s = TC.scenario(bulk_a, bulk_b, enr_db, seed, jump, HOPS, mute=mute)
        r = TrackRef(Q)
        r.run(s['mic'], s['played'])
        _RUNS[key] = r
    return _RUNS[key]


@pytest.mark.parametrize('enr_db', [10.0, 0.0])
def test_reference_follows_every_jump_with_exactly_one_move(enr_db):
    """Q = 32, the defaults (lambda 0.99, ratio 8, hold 16, patience 128, rest 0), 792 hops, the delay jumps at hop 264 and the path is
    redrawn: four jumps, three seeds each.  One lock before the jump, one move after it, none before; afterwards the main tap lies in
    0 .. 767 of the aligned path.  DESIGN.md section 18's table: the move came 30 .. 75 hops after the jump at ENR 10 dB, 47 .. 204 at
    0 dB."""
    after = []
    for a, b in JUMPS:
        for seed in (1, 2, 3):
            r = _run(a, b, enr_db, seed)
            locks, moves = r.of('lock'), r.of('move')
            assert len(locks) == 1 and locks[0][0] < JUMP and 0 <= a - HOP * locks[0][3] < 3 * HOP, (a, b, seed, r.events)
            assert len(moves) == 1 == r.moves and moves[0][0] >= JUMP and r.last_move == moves[0][0], (a, b, seed, r.events)
            assert 0 <= TC.main_tap_after_alignment(b, r.delay) < 3 * HOP, (a, b, seed, r.delay)
            after.append(moves[0][0] - JUMP)
    print('ENR %g dB: the move came %d .. %d hops after the jump (%s)' % (enr_db, min(after), max(after), after))


def test_reference_below_0_db_is_the_known_limit():
    """printed, not asserted beyond the safe failure: at ENR -5 dB a jump may not be followed within the run; the slot then stays on the
    old delay and nothing else moves"""
    for a, b in JUMPS:
        for seed in (1, 2, 3):
            r = _run(a, b, -5.0, seed)
            moves = r.of('move')
            print('ENR -5 dB, %d -> %d, seed %d: first lock at hop %s, moves %s, %d confirmations, %d give-ups'
                  % (a, b, seed, (r.of('lock') or [[None]])[0][0], [(m[0], m[3]) for m in moves], r.confirms, r.gaveups))
            assert all(m[0] >= JUMP for m in moves)


def test_reference_does_not_move_a_delay_that_is_held_or_muted():
    """2000 samples at ENR 0 dB, no jump: three seeds lock and only confirm; seed 1 again with the echo absent over hops 200 .. 599: the
    background searches give up, nothing moves, and the confirmations come back with the echo"""
    for seed in (1, 2, 3):
        r = _run(2000, 2000, 0.0, seed, jump=None)
        assert r.moves == 0 and r.confirms >= 5 and len(r.of('lock')) == 1 and 0 <= 2000 - HOP * r.delay < 3 * HOP, (seed, r.events)
    r = _run(2000, 2000, 0.0, 1, jump=None, mute=(200, 600))
    assert r.moves == 0 and r.gaveups >= 2 and [ev for ev in r.of('confirm') if ev[0] >= 600], r.events
    print('held: %s; muted 200 .. 599: %s' % ([(_run(2000, 2000, 0.0, s, jump=None).confirms) for s in (1, 2, 3)], [(e[0], e[1]) for e in r.events]))


def test_reference_never_moves_on_an_echo_free_microphone():
    """the 24 echo-free microphones behind set_delay(7), 792 hops each: a give-up every 128 hops, no confirmation, no move"""
    for name, mic, played in TC.negatives(HOPS):
        r = TrackRef(Q)
        r.set_delay(7)
        out = r.run(mic, played)
        assert (r.moves, r.confirms, r.gaveups, r.delay) == (0, 0, HOPS // 128, 7), (name, r.events)
        assert np.array_equal(out[7 * HOP:], played[:-7 * HOP]) and not out[:7 * HOP].any()


def test_the_gpu_scenarios_on_the_reference():
    """tests/test_track_gpu.py's scenarios (hold 8, patience 48, the jump at hop 110 of 300): which slots move, once each, and that the
    others do not"""
    want = {3: [1, 1, 0], 8: [1, 0, 0, 1, 0], 32: [1, 1]}
    for q, rows in TC.GPU_SCENARIOS.items():
        for slot, (a, b, enr_db, seed, taps, t60, jump) in enumerate(rows):
            s = TC.scenario(a, b, enr_db, seed, jump, TC.GPU_HOPS, taps=taps, t60=t60, shift=4001 * slot)
            r = TrackRef(q, ratio=TC.GPU_RATIO, hold=TC.GPU_HOLD, patience=TC.GPU_PATIENCE)
            r.run(s['mic'], s['played'])
            assert r.moves == want[q][slot] and len(r.of('lock')) == 1, (q, slot, r.events)
            assert all(m[0] >= jump for m in r.of('move')), (q, slot, r.events)
            if r.moves:
                assert 0 <= TC.main_tap_after_alignment(b, r.delay) < 3 * HOP


# ------------------------------------------------------------------------------------------------- TrackedEchoCanceller's bookkeeping
class _StubTrack:
    def __init__(self, S):
        import torch
        self.S, self.device, self.calls, self.resets = S, torch.device('cpu'), [], []

    def process(self, mic, played, active=None, out=None, want_moved=False):
        import torch
        self.calls.append((mic.clone(), played.clone(), None if active is None else np.array(active, dtype=bool), want_moved))
        aligned = 2.0 * played
        return (aligned, torch.tensor([0, 1, 0][:self.S], dtype=torch.uint8)) if want_moved else aligned

    def reset(self, slots):
        self.resets.append(list(slots))


class _StubAec:
    def __init__(self, S):
        import torch
        self.S, self.P, self.device, self.calls, self.resets, self.flagged, self.order = S, 4, torch.device('cpu'), [], [], [], []

    def process(self, mic, played, active=None, adapt=None, want_echo=False, out=None):
        self.order.append('process')
        self.calls.append((mic.clone(), played.clone(), None if active is None else np.array(active, dtype=bool), adapt, want_echo, out))
        return (mic - played, 3.0 * played) if want_echo else mic - played

    def reset_flagged(self, flags):
        self.order.append('reset_flagged')
        self.flagged.append(flags.clone())

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

    def reset(self, slots):
        self.resets.append(list(slots))


def test_tracked_canceller_bookkeeping_on_stubs():
    import torch
    from nele_gan_amd.aec import EchoCancellingEnhancer
    from nele_gan_amd.bulktrack import TrackedEchoCanceller
    S, W = 3, 2 * HOP
    track, aec = _StubTrack(S), _StubAec(S)
    comp = TrackedEchoCanceller(track, aec)
    assert (comp.S, comp.P, comp.device, comp.reset_on_move) == (S, 4, aec.device, True)
    g = torch.Generator().manual_seed(5)
    mic, played = torch.rand(S, W, generator=g), torch.rand(S, W, generator=g)
    # process = aec.process(mic, track.process(mic, played, active), ...), the canceller first restarted where the tracker's mask says
    res, echo = comp.process(mic, played, active=[True, False, True], adapt=[True, True, False], want_echo=True, out=('res buffer', 'echo buffer'))
    m, p, act, want_moved = track.calls[0]
    assert torch.equal(m, mic) and torch.equal(p, played) and list(act) == [True, False, True] and want_moved is True
    assert aec.order == ['reset_flagged', 'process'] and aec.flagged[0].tolist() == [0, 1, 0]
    m, p, act, adapt, want_echo, out = aec.calls[0]
    assert torch.equal(m, mic) and torch.equal(p, 2.0 * played) and list(act) == [True, False, True] and adapt == [True, True, False]
    assert want_echo is True and out == ('res buffer', 'echo buffer')
    assert torch.equal(res, mic - 2.0 * played) and torch.equal(echo, 6.0 * played)
    assert torch.equal(comp.process(mic, played), mic - 2.0 * played) and aec.calls[1][2:] == (None, None, False, None)
    assert comp.echo_path([1]) == ('path', [1])
    comp.reset([2, 0])
    assert track.resets == [[2, 0]] and aec.resets == [[2, 0]]
    # without the restart the mask is not asked for
    track, aec = _StubTrack(S), _StubAec(S)
    plain = TrackedEchoCanceller(track, aec, reset_on_move=False)
    assert torch.equal(plain.process(mic, played), mic - 2.0 * played)
    assert track.calls[0][3] is False and aec.order == ['process'] and not aec.flagged
    # inside the closed loop: it stands where an EchoCanceller does
    track, aec, rt = _StubTrack(S), _StubAec(S), _StubRt(S)
    loop = EchoCancellingEnhancer(rt, TrackedEchoCanceller(track, aec))
    clean = [torch.rand(S, W, generator=g) for _ in range(2)]
    mics = [torch.rand(S, W, generator=g) for _ in range(2)]
    out0 = loop.process(clean[0], mics[0])
    assert torch.equal(track.calls[0][1], torch.zeros(S, W)) and torch.equal(out0, clean[0] + 0.5 * mics[0] + 1.0)      # played = 0: residual = mic
    out1 = loop.process(clean[1], mics[1], active=[True, False, True])
    assert torch.equal(track.calls[1][1], out0) and list(track.calls[1][2]) == [True, False, True] and list(aec.calls[1][2]) == [True, False, True]
    assert torch.equal(out1, clean[1] + 0.5 * (mics[1] - 2.0 * out0) + 2.0)
    loop.reset([1])
    assert rt.resets == [[1]] and aec.resets == [[1]] and track.resets == [[1]]


# ------------------------------------------------------------------------------------------- the reference chain's echo reduction
def _reduction(echo, y, a, b):
    sl = slice(a * HOP, b * HOP)
    return 10.0 * np.log10(np.sum(echo[sl] ** 2) / np.sum((echo[sl] - y[sl]) ** 2))


@pytest.mark.parametrize('bulk_a,bulk_b,enr_db,seed', [(5000, 1000, 0.0, 6), (2000, 5000, 10.0, 1)])
def test_reference_chain_recovers_the_echo_reduction_after_a_move(bulk_a, bulk_b, enr_db, seed):
    """AecRef (P = 4) behind the reference tracker, one hop per call, over the 100 hops that follow the move: with the canceller begun
    again on the hop of the move, without, and behind the BulkRef that never moves.  DESIGN.md section 18: 5.85 / 3.82 / -0.30 dB on
    5000 -> 1000 at ENR 0 dB, 5.85 / 4.08 / -0.59 dB on 2000 -> 5000 at ENR 10 dB.  Required: tracked ends at least as well as
    untracked; reset_on_move defaults to True because the restart is not worse than none"""
    P = 4
    s = TC.scenario(bulk_a, bulk_b, enr_db, seed, JUMP, HOPS)
    tr, aec, aec_kept, y, y_kept, move = TrackRef(Q), AecRef(P), AecRef(P), [], [], None
    for k in range(HOPS):
        d = s['mic'][k * HOP:(k + 1) * HOP]
        al, moved = tr.hop(d, s['played'][k * HOP:(k + 1) * HOP])
        if moved:
            aec, move = AecRef(P), k
        y.append(aec.hop(d, al)[1])
        y_kept.append(aec_kept.hop(d, al)[1])
    assert move is not None and tr.moves == 1 and move + 100 <= HOPS
    _, y_unt = AecRef(P).run(s['mic'], BulkRef(Q).run(s['mic'], s['played'])[0])
    reset, kept, untracked = (_reduction(s['echo'], v, move, move + 100) for v in (np.concatenate(y), np.concatenate(y_kept), y_unt))
    print('%d -> %d, ENR %g dB, moved at hop %d, hops %d .. %d: restarted %.2f dB, weights kept %.2f dB, untracked %.2f dB'
          % (bulk_a, bulk_b, enr_db, move, move, move + 99, reset, kept, untracked))
    assert reset >= untracked and kept >= untracked
    assert reset >= kept                                                          # what keeps reset_on_move=True the default
