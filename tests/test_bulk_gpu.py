"""GPU: the bulk-delay search (nele_gan_amd/bulkdelay.py, csrc/bulkdelay.hip) against tests/bulk_ref.py - the float64 numpy restatement
of DESIGN.md section 16 - its streaming contract (grouping, batch, slots, skipped calls, reset, set_delay: bitwise), and the composite
with the echo canceller, alone, in the closed loop around RealtimeEnhancer and on the command line.

Decisions are integers, so a parity scenario must not sit on a threshold: on the reference, asserted here for every scenario,
|conf / ratio - 1| >= 1e-6 at every evaluated hop and 1 - e_second / e_first >= 1e-6 whenever the block leads by the ratio.
Bounds: lock hop and delay equal; aligned bit-equal (zeros, then float32 copies); e and conf of nele_bulk_status, read after every
call (the one in which the lock falls and the last one included), within 1e-9 max_q e_q of the reference's (conf also within 1e-9 of
itself, relatively): the float64 transforms agree to about 1e-15, the squares and the decayed sums leave orders of magnitude of room,
while a wrong ring index, conjugate, constraint or block costs more than 1e-2.
Measured on an MI355X (largest |e - e_ref| / max_q e_q, then |conf - conf_ref| / max_q e_q): 3.6e-16 and 2.6e-17 at (B, Q) = (1, 2);
3.3e-16 and 8.1e-17 at (3, 3), the unpaired block; 5.3e-16 and 1.4e-16 at (2, 32); 7.3e-16 and 7.3e-17 at (1, 64); 5.9e-16 and 1.4e-16
at (5, 8) with ragged active masks; 7.5e-16 and 5.9e-17 for an echo-free microphone after 264 hops of search.  Composite on bulk 5000 at
ENR 0 dB, hops 164 .. 263: reference 7.54 dB, GPU 7.54 dB, the plain canceller at P = 8 -0.28 dB."""
import numpy as np
import pytest

import aec_cases as C
import bulk_cases as BC
from aec_ref import AecRef
from bulk_ref import HOP, BulkRef

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from weights_recipe import seeded_state_arrays  # noqa: E402

SENTINEL = -7.25
HOPS = 264
RATIO = 8.0
# Q -> per slot (bulk, ENR dB, path seed, taps, T60); slot i's far end is shifted by 4001 i
SCENARIOS = {
    2: [(300, 10.0, 21, 150, 0.02)],
    3: [(100, 10.0, 31, 200, 0.03), (400, 10.0, 32, 200, 0.03), (600, 0.0, 33, 150, 0.03)],
    8: [(40, 10.0, 81, 700, 0.08), (700, 10.0, 82, 300, 0.04), (1000, 10.0, 83, 700, 0.08), (1500, 10.0, 84, 300, 0.04), (1900, 10.0, 85, 700, 0.08)],
    32: [(5000, 0.0, 6, 700, 0.08), (7000, 10.0, 5, 700, 0.08)],
    64: [(15000, 10.0, 64, 700, 0.08)],
}
_SCEN, _REF = {}, {}


def scen(Q, slot):
    if (Q, slot) not in _SCEN:
        bulk, enr_db, seed, taps, t60 = SCENARIOS[Q][slot]
        _SCEN[(Q, slot)] = BC.scenario(bulk, enr_db, seed, taps=taps, t60=t60, shift=4001 * slot)
    return _SCEN[(Q, slot)]


def ref_run(Q, slot):
    """(aligned, lock hop, BulkRef) of the reference on scen(Q, slot): computed once, shared, never changed.  Asserts that no decision
    of the scenario sits on a threshold."""
    if (Q, slot) not in _REF:
        s = scen(Q, slot)
        r = BulkRef(Q, ratio=RATIO)
        al, lock = r.run(s['mic'], s['played'])
        margin = min(abs(l[3] / RATIO - 1.0) for l in r.log)
        gap = min([1.0 - l[4] for l in r.log if l[2]] or [1.0])
        print('reference Q %d slot %d: lock hop %s, delay %d, min |conf / ratio - 1| %.3g, min top-two gap %.3g' % (Q, slot, lock, r.delay, margin, gap))
        assert margin >= 1e-6 and gap >= 1e-6, (Q, slot, margin, gap)
        _REF[(Q, slot)] = (al, lock, r)
    return _REF[(Q, slot)]


def _bulk(B, Q, **kw):
    from nele_gan_amd.bulkdelay import BulkDelay
    return BulkDelay(B, blocks=Q, ratio=RATIO, **kw)


def _record(bd, slot):
    from nele_gan_amd import _lib
    rec = int(_lib.lib.nele_bulk_stream_record_bytes(bd.Q))
    header = bd.nbytes - bd.S * rec
    return bd.state[header + slot * rec:header + (slot + 1) * rec].clone()


def _status(bd):
    return {k: v.cpu().numpy() for k, v in bd.status().items()}


def feed(bd, mics, playeds, group, slots=None, after=None):
    """all hops of the given streams through ``bd`` (in ``slots``, default 0 ..), ``group`` hops per call at most -> aligned [n, L] on
    the host; after(hops fed so far): called behind every call"""
    slots = list(range(len(mics))) if slots is None else slots
    L = len(mics[0])
    out = []
    for a in range(0, L, group * HOP):
        b = min(L, a + group * HOP)
        D = np.zeros((bd.S, b - a), np.float32)
        X = np.zeros((bd.S, b - a), np.float32)
        act = np.zeros(bd.S, bool)
        for i, s in enumerate(slots):
            D[s], X[s], act[s] = mics[i][a:b], playeds[i][a:b], True
        y = bd.process(torch.from_numpy(D), torch.from_numpy(X), active=None if act.all() else act)
        out.append(y[slots].cpu().numpy())
        if after is not None:
            after(b // HOP)
    return np.concatenate(out, axis=1)


def check_status(tag, st, slot, ref, fed, worst):
    """nele_bulk_status of ``slot`` after ``fed`` hops against the reference's log (ref: what ref_run returns, or (None, lock, BulkRef));
    worst: [e, conf] largest ratios so far"""
    _, lock, r = ref
    n_ref = fed if lock is None else min(fed, lock + 1)                           # no search work after the lock
    assert st['hops_searched'][slot] == n_ref, (tag, fed, st['hops_searched'][slot], n_ref)
    assert st['delay'][slot] == (r.delay if lock is not None and fed > lock else -1), (tag, fed)
    log = [l for l in r.log if l[0] <= n_ref]
    if not log:
        assert not st['energies'][slot].any() and st['conf'][slot] == 0.0
        return
    _, qs, ok, conf, _, e = log[-1]
    scale = float(e.max())
    de = float(np.abs(st['energies'][slot] - e).max() / scale)
    dc = float(abs(st['conf'][slot] - conf))
    worst[0], worst[1] = max(worst[0], de), max(worst[1], dc / scale)
    assert de <= 1e-9, (tag, fed, de)
    assert dc <= 1e-9 * scale and dc <= 1e-9 * abs(conf), (tag, fed, dc, scale, conf)
    assert int(np.argmax(st['energies'][slot])) == qs


def check_parity(tag, aligned, st, slot, Q, ref_slot):
    al_ref, lock, r = ref_run(Q, ref_slot)
    assert st['delay'][slot] == r.delay, (tag, st['delay'][slot], r.delay)
    nz = np.nonzero(aligned.reshape(-1, HOP).any(axis=1))[0]
    got_lock = None if st['delay'][slot] < 0 else int(st['hops_searched'][slot]) - 1
    assert got_lock == lock, (tag, got_lock, lock)
    assert np.array_equal(aligned, al_ref), tag
    assert lock is None or (len(nz) and nz[0] >= lock)


# -------------------------------------------------------------------------------------------------------- parity against the reference
@pytest.mark.parametrize('B,Q', [(1, 2), (3, 3), (2, 32), (1, 64)])
def test_parity_with_the_reference(B, Q):
    """every slot of the batch against the reference on its own scenario, 11 hops per call, the status compared after every call;
    (3, 3): the unpaired block, which slot 2's echo arrives in"""
    ss = [scen(Q, i) for i in range(B)]
    refs = [ref_run(Q, i) for i in range(B)]
    assert all(r[1] is not None for r in refs)                                    # every scenario locks: there is an `aligned` to compare
    bd = _bulk(B, Q)
    worst = [0.0, 0.0]

    def after(fed):
        st = _status(bd)
        for i in range(B):
            check_status('B %d Q %d slot %d' % (B, Q, i), st, i, refs[i], fed, worst)

    aligned = feed(bd, [s['mic'] for s in ss], [s['played'] for s in ss], 11, after=after)
    st = _status(bd)
    assert np.array_equal(st['delay'], bd.delays().cpu().numpy())
    for i in range(B):
        check_parity('B %d Q %d slot %d' % (B, Q, i), aligned[i], st, i, Q, i)
    print('B %d Q %d: delays %s, worst |e - e_ref| / max e %.3g, worst |conf - conf_ref| / max e %.3g (bound 1e-9)' % (B, Q, st['delay'].tolist(), worst[0], worst[1]))


def test_parity_with_ragged_active_masks():
    """B = 5, Q = 8: each call brings 8 hops to a random subset of the slots, the others are inactive and their input rows hold NaN - a
    slot that is read while inactive poisons its state"""
    B, Q, G = 5, 8, 8
    ss = [scen(Q, i) for i in range(B)]
    refs = [ref_run(Q, i) for i in range(B)]
    bd = _bulk(B, Q)
    rng = np.random.RandomState(7)
    pos = np.zeros(B, int)
    got = [[] for _ in range(B)]
    worst = [0.0, 0.0]
    while (pos < HOPS).any():
        act = (rng.rand(B) < 0.6) & (pos < HOPS)
        if not act.any():
            continue
        D = np.full((B, G * HOP), np.nan, np.float32)
        X = np.full((B, G * HOP), np.nan, np.float32)
        for i in np.nonzero(act)[0]:
            D[i], X[i] = ss[i]['mic'][pos[i] * HOP:(pos[i] + G) * HOP], ss[i]['played'][pos[i] * HOP:(pos[i] + G) * HOP]
        y = bd.process(torch.from_numpy(D), torch.from_numpy(X), active=act).cpu().numpy()
        for i in np.nonzero(act)[0]:
            got[i].append(y[i])
            pos[i] += G
        st = _status(bd)
        for i in range(B):
            if pos[i]:
                check_status('ragged slot %d' % i, st, i, refs[i], int(pos[i]), worst)
    assert list(bd.hops) == [HOPS] * B
    st = _status(bd)
    for i in range(B):
        check_parity('ragged slot %d' % i, np.concatenate(got[i]), st, i, Q, i)
    print('ragged B 5 Q 8: delays %s, worst |e - e_ref| / max e %.3g, conf %.3g' % (st['delay'].tolist(), worst[0], worst[1]))


def test_a_slot_without_an_echo_keeps_searching():
    """the time-reversed far end as microphone: zeros out, delay -1, the status still within the bound after 264 hops of search"""
    far, _ = C.far_and_near()
    mic, played = far[::-1].astype(np.float32), far.astype(np.float32)
    r = BulkRef(8, ratio=RATIO)
    al_ref, lock = r.run(mic, played)
    assert lock is None and min(abs(l[3] / RATIO - 1.0) for l in r.log) >= 1e-6
    bd = _bulk(1, 8)
    aligned = feed(bd, [mic], [played], 24)
    st, worst = _status(bd), [0.0, 0.0]
    assert not aligned.any() and st['delay'][0] == -1
    check_status('no echo', st, 0, (al_ref, lock, r), HOPS, worst)
    print('no echo, Q 8, 264 hops searched: worst |e - e_ref| / max e %.3g, conf %.3g' % tuple(worst))


# ---------------------------------------------------------------------------------------------------------------- bitwise invariances
def _full_run(bd, s, group, slot=0, others=None):
    """-> (aligned, delay, status arrays of the slot, its record)"""
    if others is None:
        aligned = feed(bd, [s['mic']], [s['played']], group, slots=[slot])[0]
    else:
        ss = list(others)
        aligned = feed(bd, [x['mic'] for x in ss], [x['played'] for x in ss], group)[slot]
    st = _status(bd)
    return aligned, bd.delays().cpu().numpy()[slot], {k: v[slot].copy() for k, v in st.items()}, _record(bd, slot).cpu().numpy()


def _same(a, b):
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    for k in a[2]:
        assert np.array_equal(a[2][k], b[2][k]), k
    assert np.array_equal(a[3], b[3])


@pytest.mark.parametrize('Q', [3, 8])
def test_hop_grouping_and_batch_do_not_change_a_slot(Q):
    """one hop per call = 7 per call (the lock falls inside a call) = all 264 at once; alone = in slot 3 of B = 5 beside other streams:
    aligned, delay, status and every byte of the record"""
    slot_scen = {3: 2, 8: 4}[Q]
    s = scen(Q, slot_scen)
    lock = ref_run(Q, slot_scen)[1]
    assert lock is not None and lock % 7 != 6                                     # the lock does not fall on the last hop of a call of 7
    runs = [_full_run(_bulk(1, Q), s, group) for group in (1, 7, HOPS)]
    assert runs[0][1] >= 0 and runs[0][0].any()
    for r in runs[1:]:
        _same(r, runs[0])
    others = [scen(8, i) for i in range(5)]
    others[3] = s
    _same(_full_run(_bulk(5, Q), s, 5, slot=3, others=others), runs[0])


def test_inactive_slots_are_neither_read_nor_written():
    B, Q, n0, n1 = 3, 8, 60, 6
    ss = [scen(Q, i) for i in range(B)]
    mics, pls = [s['mic'] for s in ss], [s['played'] for s in ss]
    bd = _bulk(B, Q)
    feed(bd, [m[:n0 * HOP] for m in mics], [p[:n0 * HOP] for p in pls], 12)
    before, st_before = _record(bd, 1), _status(bd)
    # a call that skips slot 1: NaN inputs there, a sentinel-filled output and delay_hops
    D = np.stack([m[n0 * HOP:(n0 + n1) * HOP] for m in mics])
    X = np.stack([p[n0 * HOP:(n0 + n1) * HOP] for p in pls])
    D[1], X[1] = np.nan, np.nan
    out = torch.full((B, n1 * HOP), SENTINEL, device='cuda')
    bd.process(torch.from_numpy(D), torch.from_numpy(X), active=[True, False, True], out=out)
    assert (out[1] == SENTINEL).all() and not (out[0] == SENTINEL).any() and not (out[2] == SENTINEL).any()
    assert torch.equal(_record(bd, 1), before)
    st = _status(bd)
    for k in st:
        assert np.array_equal(st[k][1], st_before[k][1]), k
    # slot 1 goes on where it was: equal to a run that never saw the skipped call
    y1 = feed(bd, [mics[1][n0 * HOP:]], [pls[1][n0 * HOP:]], 17, slots=[1])
    alone = _bulk(1, Q)
    ya = feed(alone, [mics[1]], [pls[1]], HOPS)
    assert np.array_equal(y1[0], ya[0][n0 * HOP:]) and ya.any()
    assert np.array_equal(_record(bd, 1).cpu().numpy(), _record(alone, 0).cpu().numpy())


def test_hop_reports_the_delays_of_the_active_slots():
    """nele_bulk_hop's own delay_hops output (the class does not ask for it): active slots' delays, inactive entries left as they were"""
    from nele_gan_amd._lib import c_longlong, call, ptr, stream
    B, Q = 3, 8
    ss = [scen(Q, i) for i in range(B)]
    bd = _bulk(B, Q)
    locks = {i: ref_run(Q, i)[1] for i in (0, 2)}
    nh = min(locks.values()) + 1                                                  # one of the two active slots has locked by then, the other has not
    want = {i: ref_run(Q, i)[2].delay if locks[i] < nh else -1 for i in (0, 2)}
    assert sorted(v >= 0 for v in want.values()) == [False, True]
    n = nh * HOP
    mic = torch.from_numpy(np.stack([s['mic'][:n] for s in ss])).cuda()
    pl = torch.from_numpy(np.stack([s['played'][:n] for s in ss])).cuda()
    dh = torch.full((B,), 77, dtype=torch.int32, device='cuda')
    out = torch.empty_like(mic)
    act = torch.tensor([1, 0, 1], dtype=torch.uint8, device='cuda')
    call('nele_bulk_hop', ptr(bd.state), c_longlong(bd.nbytes), B, Q, ptr(mic), ptr(pl), ptr(act), n // HOP, bd.lam, bd.ratio, bd.hold, ptr(out),
         ptr(dh), stream())
    assert dh.tolist() == [want[0], 77, want[2]]
    assert bd.delays().tolist() == [want[0], -1, want[2]]


def test_reset_restarts_one_slot_and_leaves_the_others():
    B, Q, n0 = 3, 8, 100
    ss = [scen(Q, i) for i in range(B)]
    mics, pls = [s['mic'] for s in ss], [s['played'] for s in ss]
    rest = HOPS - n0
    fresh = _bulk(1, Q)
    yf = feed(fresh, [mics[1][:rest * HOP]], [pls[1][:rest * HOP]], 41)
    assert ref_run(Q, 1)[1] < min(n0, rest)                                       # slot 1 has locked before the reset, and locks again after it

    def run(with_reset):
        bd = _bulk(B, Q)
        feed(bd, [m[:n0 * HOP] for m in mics], [p[:n0 * HOP] for p in pls], 9)
        if with_reset:
            assert bd.delays()[1].item() >= 0
            bd.reset([1])
            assert bd.delays().tolist()[1] == -1 and not _record(bd, 1).any() and bd.delays()[0].item() >= 0
        m2 = [m[n0 * HOP:] for m in mics]
        p2 = [p[n0 * HOP:] for p in pls]
        if with_reset:
            m2[1], p2[1] = mics[1][:rest * HOP], pls[1][:rest * HOP]
        y = feed(bd, m2, p2, 13)
        return y, [_record(bd, i).cpu().numpy() for i in range(B)]

    y, recs = run(True)
    assert np.array_equal(y[1], yf[0]) and yf.any() and np.array_equal(recs[1], _record(fresh, 0).cpu().numpy())
    y_, recs_ = run(False)
    for s in (0, 2):
        assert np.array_equal(y[s], y_[s]) and np.array_equal(recs[s], recs_[s])


def test_set_delay_shifts_played_by_whole_hops():
    """set_delay(h) on fresh slots, h = 0, 1 and Q - 1: aligned = played late by 256 h samples behind leading zeros, exactly, and no
    search runs; an out-of-range h (through the C entry point: the class raises) changes nothing"""
    from nele_gan_amd._lib import c_longlong, call, ptr, stream
    B, Q, nh = 4, 5, 12
    rng = np.random.default_rng(3)
    mic = rng.standard_normal((B, nh * HOP)).astype(np.float32)
    played = rng.standard_normal((B, nh * HOP)).astype(np.float32)
    bd = _bulk(B, Q)
    bd.set_delay([0, 1, 2], [0, 1, Q - 1])
    before = _record(bd, 3)
    flags = torch.tensor([0, 0, 0, 1], dtype=torch.uint8, device='cuda')
    for bad in (Q, -1, 1 << 30):
        hops = torch.tensor([0, 0, 0, bad], dtype=torch.int32, device='cuda')
        call('nele_bulk_set_delay', ptr(bd.state), c_longlong(bd.nbytes), B, Q, ptr(flags), ptr(hops), stream())
    assert torch.equal(_record(bd, 3), before) and bd.delays().tolist() == [0, 1, Q - 1, -1]
    with pytest.raises(ValueError, match='hops'):
        bd.set_delay([3], Q)
    y = feed(bd, list(mic), list(played), 5)
    for slot, h in ((0, 0), (1, 1), (2, Q - 1)):
        want = np.concatenate([np.zeros(h * HOP, np.float32), played[slot]])[:nh * HOP]
        assert np.array_equal(y[slot], want), slot
    st = _status(bd)
    assert st['hops_searched'].tolist() == [0, 0, 0, nh] and st['delay'].tolist() == [0, 1, Q - 1, -1] and not y[3].any()


def test_a_locked_slot_runs_the_delay_line_and_leaves_its_search_state():
    """B = 2, Q = 3, hold 8: slot 0 locks (where the reference does), slot 1 searches on beside it.  Through 8 more hops in two calls
    slot 0's hops_searched, energies and conf are the bits they were at the lock, and so is its record apart from the delay line and
    its head: a plain search that comes into a call locked neither loads nor stores search state.  aligned is `played` late by the
    delay."""
    B, Q, hold, extra = 2, 3, 8, 8
    ss = [scen(Q, i) for i in range(B)]
    r = BulkRef(Q, ratio=RATIO, hold=hold)
    _, lock = r.run(ss[0]['mic'][:32 * HOP], ss[0]['played'][:32 * HOP])
    assert lock is not None and r.delay >= 0
    n = lock + 1
    assert n + extra <= 40
    mics, pls = [s['mic'][:(n + extra) * HOP] for s in ss], [s['played'][:(n + extra) * HOP] for s in ss]
    bd = _bulk(B, Q, hold=hold)
    y0 = feed(bd, [m[:n * HOP] for m in mics], [p[:n * HOP] for p in pls], 7)
    at_lock, rec = _status(bd), _record(bd, 0).cpu().numpy()
    assert at_lock['delay'].tolist() == [r.delay, -1] and at_lock['hops_searched'].tolist() == [n, n] and at_lock['energies'][0].all()
    y1 = feed(bd, [m[n * HOP:] for m in mics], [p[n * HOP:] for p in pls], extra // 2)
    st, rec1 = _status(bd), _record(bd, 0).cpu().numpy()
    for k in ('delay', 'hops_searched', 'energies', 'conf'):
        assert np.array_equal(st[k][0], at_lock[k][0]), k
    assert st['delay'][1] == -1 and st['hops_searched'][1] == n + extra          # the neighbour went on searching in the same calls
    line = slice(6144, 6144 + 4 * HOP * Q)                                       # DESIGN.md section 16's record: the delay line; int [1] is its head
    assert np.array_equal(rec[:4], rec1[:4]) and np.array_equal(rec[8:line.start], rec1[8:line.start])
    assert np.array_equal(rec[line.stop:], rec1[line.stop:]) and not np.array_equal(rec[line], rec1[line])
    y = np.concatenate([y0, y1], axis=1)
    want = np.concatenate([np.zeros(r.delay * HOP, np.float32), pls[0]])[:(n + extra) * HOP]
    want[:lock * HOP] = 0.0
    assert np.array_equal(y[0], want) and y[0].any() and not y[1].any()


# ---------------------------------------------------------------------------------------------------------------------- the composite
def _reduction(echo, y, a=164, b=264):
    sl = slice(a * HOP, b * HOP)
    return 10.0 * np.log10(np.sum(echo[sl] ** 2) / np.sum((echo[sl] - y[sl]) ** 2))


def test_aligned_canceller_is_the_chain_by_hand_and_restores_the_reduction():
    """B = 2, Q = 32, P = 4, 8 hops per call: AlignedEchoCanceller = BulkDelay then EchoCanceller by hand, bit for bit; on bulk 5000 at
    ENR 0 dB its echo reduction over hops 164 .. 263 is within 0.01 dB of the reference composite's and at least 5 dB above the plain
    canceller's at P = 8"""
    from nele_gan_amd.aec import EchoCanceller
    from nele_gan_amd.bulkdelay import AlignedEchoCanceller
    B, Q, P, G = 2, 32, 4, 8
    ss = [scen(Q, i) for i in range(B)]
    mic = np.stack([s['mic'] for s in ss])
    pl = np.stack([s['played'] for s in ss])
    comp = AlignedEchoCanceller(_bulk(B, Q), EchoCanceller(B, partitions=P))
    hb, ha = _bulk(B, Q), EchoCanceller(B, partitions=P)
    plain = EchoCanceller(B, partitions=8)
    echo, echo8 = [], []
    for a in range(0, HOPS * HOP, G * HOP):
        d, x = torch.from_numpy(mic[:, a:a + G * HOP].copy()).cuda(), torch.from_numpy(pl[:, a:a + G * HOP].copy()).cuda()
        r1, y1 = comp.process(d, x, want_echo=True)
        r2, y2 = ha.process(d, hb.process(d, x), want_echo=True)
        assert torch.equal(r1, r2) and torch.equal(y1, y2), a
        echo.append(y1.cpu().numpy())
        echo8.append(plain.process(d, x, want_echo=True)[1].cpu().numpy())
    echo, echo8 = np.concatenate(echo, axis=1).astype(np.float64), np.concatenate(echo8, axis=1).astype(np.float64)
    assert comp.bulk.delays().tolist() == [ref_run(Q, 0)[2].delay, ref_run(Q, 1)[2].delay]
    assert torch.equal(comp.echo_path(), ha.echo_path()) and list(comp.aec.hops) == list(comp.bulk.hops) == [HOPS] * B
    _, y_ref = AecRef(P).run(ss[0]['mic'], ref_run(Q, 0)[0])
    red_ref, red_gpu, red_plain = _reduction(ss[0]['echo'], y_ref), _reduction(ss[0]['echo'], echo[0]), _reduction(ss[0]['echo'], echo8[0])
    print('bulk 5000, ENR 0 dB, hops 164 .. 263: reference composite %.2f dB, GPU composite %.2f dB, GPU plain P = 8 %.2f dB' % (red_ref, red_gpu, red_plain))
    assert abs(red_gpu - red_ref) <= 0.01
    assert red_gpu >= red_plain + 5.0


def _generator():
    from nele_gan_amd import model
    G = model.Generator_Conv1D_cLN()
    sd = G.state_dict()
    arrs = seeded_state_arrays([(k, tuple(v.shape)) for k, v in sd.items()], 101)
    G.load_state_dict({k: torch.from_numpy(v) for k, v in arrs.items()})
    return G.cuda()


def test_closed_loop_around_the_realtime_enhancer():
    """EchoCancellingEnhancer(rt, AlignedEchoCanceller(bulk, aec)) against the three objects chained by hand, in lockstep on one
    microphone signal (noise plus the echo, 600 samples of bulk delay behind the loop's own call, of what the loop itself returned):
    B = 2, Q = 8, P = 2, 4 hops per call, 40 calls and a tail of 100 samples; bit-identical, finish included"""
    from nele_gan_amd.aec import EchoCanceller, EchoCancellingEnhancer
    from nele_gan_amd.bulkdelay import AlignedEchoCanceller
    from nele_gan_amd.realtime import RealtimeEnhancer
    B, Q, P, NH, CALLS, TAIL = 2, 8, 2, 4, 40, 100
    W, L = NH * HOP, NH * HOP * CALLS
    G = _generator()
    ss = [scen(Q, i) for i in range(B)]
    clean = np.stack([s['played'] for s in ss])
    noise = 0.1 * np.stack([s['noise'] for s in ss])
    hs = [BC.path(200 + i, 200, 0.03, 600) for i in range(B)]

    def rt():
        return RealtimeEnhancer(G=G, streams=B, precision='f32')

    loop = EchoCancellingEnhancer(rt(), AlignedEchoCanceller(_bulk(B, Q), EchoCanceller(B, partitions=P)))
    hand_rt, hand_bulk, hand_aec = rt(), _bulk(B, Q), EchoCanceller(B, partitions=P)
    ls = np.zeros((B, L + 2 * W))                                                 # the loudspeaker: out of call c at columns [(c + 1) W, (c + 2) W)
    played = torch.zeros((B, W), device='cuda')

    def mic_of(c, width):
        a, b = c * W, c * W + width
        echo = np.stack([np.convolve(ls[i, :b], hs[i])[a:b] for i in range(B)])
        return (noise[:, a:b] + echo).astype(np.float32)

    for c in range(CALLS):
        m = torch.from_numpy(mic_of(c, W))
        cl = torch.from_numpy(clean[:, c * W:(c + 1) * W].copy())
        out = loop.process(cl, m)
        res = hand_aec.process(m, hand_bulk.process(m, played))
        played = hand_rt.process(cl, res)
        assert torch.equal(out, played), c
        ls[:, (c + 1) * W:(c + 2) * W] = out.cpu().numpy()
    ct, mt = np.zeros((B, HOP), np.float32), np.zeros((B, HOP), np.float32)
    ct[:, :TAIL], mt[:, :TAIL] = clean[:, L:L + TAIL], mic_of(CALLS, TAIL)
    last = loop.finish([0, 1], ct, mt, [TAIL, TAIL])
    m = torch.from_numpy(mt).cuda()
    res = hand_aec.process(m, hand_bulk.process(m, played[:, :HOP].contiguous()))
    assert torch.equal(last, hand_rt.finish([0, 1], ct, res.cpu(), [TAIL, TAIL]))
    assert list(loop.rt.emitted) == [L, L]
    assert torch.equal(loop.aec.bulk.delays(), hand_bulk.delays())
    print('closed loop: delays found %s (600 samples of bulk delay; -1 = still searching)' % loop.aec.bulk.delays().tolist())
    loop.reset([1])
    assert loop.aec.bulk.delays().tolist()[1] == -1 and not loop.aec.echo_path([1]).any()


# ----------------------------------------------------------------------------------------------------------------------- command line
def test_command_line(tmp_path, capsys):
    from nele_gan_amd import aec as A
    from nele_gan_amd import dataio
    from nele_gan_amd.bulkdelay import AlignedEchoCanceller
    Q, P = 8, 3
    s = scen(Q, 2)
    L = 120 * HOP + 100
    mic_path, pl_path, out_path, out_b = (str(tmp_path / n) for n in ('mic.wav', 'played.wav', 'out.wav', 'out_bulk.wav'))
    dataio.write_wav_pcm16(mic_path, s['mic'][:L])
    dataio.write_wav_pcm16(pl_path, s['played'][:L])
    mic, _ = dataio.read_wav(mic_path)
    pl, _ = dataio.read_wav(pl_path)
    n = L // HOP * HOP
    d, x = torch.from_numpy(mic[None, :n].copy()), torch.from_numpy(pl[None, :n].copy())

    def pcm(res):
        return dataio.pcm16_quantise(res).astype(np.float32) / np.float32(32768.0)

    # without the option: the plain canceller, and not a word about a bulk delay
    assert A.main(['--mic', mic_path, '--played', pl_path, '--out', out_path, '--partitions', str(P)]) == 0
    said = capsys.readouterr().out
    assert 'bulk' not in said and '%d partitions' % P in said
    out, _ = dataio.read_wav(out_path)
    assert np.array_equal(out[:n], pcm(A.EchoCanceller(1, partitions=P).process(d, x)[0].cpu().numpy()))
    # with it: the composite, and the delay found
    assert A.main(['--mic', mic_path, '--played', pl_path, '--out', out_b, '--partitions', str(P), '--bulk-blocks', str(Q)]) == 0
    said = capsys.readouterr().out
    comp = AlignedEchoCanceller(_bulk(1, Q), A.EchoCanceller(1, partitions=P))
    res = comp.process(d, x)[0].cpu().numpy()
    found = comp.bulk.delays().tolist()[0]
    assert found >= 0 and 'bulk delay: %d hops' % found in said
    out2, _ = dataio.read_wav(out_b)
    assert np.array_equal(out2[:n], pcm(res)) and not np.array_equal(out2, out)
    # a microphone without an echo: none found
    far, _ = C.far_and_near()
    dataio.write_wav_pcm16(mic_path, far[::-1][:L].astype(np.float32))
    assert A.main(['--mic', mic_path, '--played', pl_path, '--out', out_b, '--bulk-blocks', str(Q)]) == 0
    assert 'bulk delay: none found in %d blocks' % Q in capsys.readouterr().out
    with pytest.raises(SystemExit):
        A.main(['--mic', mic_path, '--played', pl_path, '--out', out_b, '--bulk-blocks', '65'])
