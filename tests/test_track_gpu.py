"""GPU: the delay tracker (nele_gan_amd/bulktrack.py, the tracking mode of csrc/bulkdelay.hip) against tests/track_ref.py - the numpy restatement of DESIGN.md
section 18 - through jumps of the bulk delay; its first search and its background searches against nele_bulk_hop (bitwise: they are
the same code); its streaming contract (grouping, batch, slots, skipped calls, reset, set_delay: bitwise); rest and patience; and the
composite with the echo canceller, alone and on the command line.

Decisions are integers, so a parity scenario must not sit on a threshold: on the reference, asserted here for every scenario,
|conf / ratio - 1| >= 1e-6 at every evaluated hop and 1 - e_second / e_first >= 1e-6 whenever the block leads by the ratio.
Bounds: aligned bit-equal; delay, hop count, age, sleep, moves, confirms, gave-ups and last_move of nele_track_status equal after every
call, the `moved` mask of every call equal; e and conf within the bounds of tests/test_bulk_gpu.py's parity test (1e-9 max_q e_q; conf
also within 1e-9 of itself, relatively).  hold 8, patience 48, the jump at hop 110 of 300: what the reference then does, slot by slot,
is in tests/test_track_cpu.py (test_the_gpu_scenarios_on_the_reference).
Measured on an MI355X (largest |e - e_ref| / max_q e_q, then |conf - conf_ref| / max_q e_q): 6.1e-16 and 6.1e-16 at (B, Q) = (3, 3);
9.0e-16 and 2.2e-16 at (5, 8); 1.1e-15 and 3.9e-16 at (2, 32); 7.8e-16 and 4.1e-16 at (5, 8) with ragged active masks.  Composite on
5000 -> 1000 samples at ENR 0 dB, hops 150 .. 299: reference chain 5.74 dB, GPU 5.74 dB; untracked reference -0.26 dB, GPU -0.26 dB."""
import numpy as np
import pytest

import aec_cases as C
import bulk_cases as BC
import track_cases as TC
from aec_ref import AecRef
from bulk_ref import HOP, BulkRef
from track_ref import TrackRef

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

HOLD, HOPS, JUMP, PATIENCE, RATIO, SCENARIOS = TC.GPU_HOLD, TC.GPU_HOPS, TC.GPU_JUMP, TC.GPU_PATIENCE, TC.GPU_RATIO, TC.GPU_SCENARIOS

SENTINEL = -7.25
INTS = ('delay', 'hops', 'age', 'sleep', 'moves', 'confirms', 'gaveups', 'last_move')
_SCEN, _REF = {}, {}


def scen(Q, slot):
    if (Q, slot) not in _SCEN:
        a, b, enr_db, seed, taps, t60, jump = SCENARIOS[Q][slot]
        _SCEN[(Q, slot)] = TC.scenario(a, b, enr_db, seed, jump, HOPS, taps=taps, t60=t60, shift=4001 * slot)
    return _SCEN[(Q, slot)]


def ref_of(mic, played, Q, rest=0, set_delay=None, patience=PATIENCE):
    """the reference over whole hops -> dict: aligned, moved [hops] bool, ints [hops][8] (INTS after every hop), e [hops][Q], conf
    [hops], ref (the TrackRef).  Asserts that no decision sits on a threshold."""
    r = TrackRef(Q, ratio=RATIO, hold=HOLD, patience=patience, rest=rest)
    if set_delay is not None:
        r.set_delay(set_delay)
    out, moved, ints, es, confs = [], [], [], [], []
    for i in range(0, len(mic), HOP):
        y, m = r.hop(mic[i:i + HOP], played[i:i + HOP])
        out.append(y)
        moved.append(m)
        ints.append((r.delay, r.hops, r.age, r.sleep, r.moves, r.confirms, r.gaveups, r.last_move))
        es.append(r.e)
        confs.append(r.conf)
    margin = min([abs(l[4] / RATIO - 1.0) for l in r.log] or [1.0])
    gap = min([1.0 - l[5] for l in r.log if l[3]] or [1.0])
    assert margin >= 1e-6 and gap >= 1e-6, (margin, gap)
    return {'aligned': np.concatenate(out), 'moved': np.array(moved), 'ints': np.array(ints), 'e': np.array(es), 'conf': np.array(confs), 'ref': r}


def ref_run(Q, slot, rest=0):
    """ref_of on scen(Q, slot): computed once, shared, never changed"""
    if (Q, slot, rest) not in _REF:
        s = scen(Q, slot)
        _REF[(Q, slot, rest)] = ref_of(s['mic'], s['played'], Q, rest=rest)
        print('reference Q %d slot %d rest %d: %s' % (Q, slot, rest, [(e[0], e[1], e[3]) for e in _REF[(Q, slot, rest)]['ref'].events]))
    return _REF[(Q, slot, rest)]


def _track(B, Q, **kw):
    from nele_gan_amd.bulktrack import TrackingBulkDelay
    return TrackingBulkDelay(B, blocks=Q, ratio=RATIO, **dict({'hold': HOLD, 'patience': PATIENCE}, **kw))


def _bulk(B, Q):
    from nele_gan_amd.bulkdelay import BulkDelay
    return BulkDelay(B, blocks=Q, ratio=RATIO, hold=HOLD)


def _record(tr, slot):
    from nele_gan_amd import _lib
    rec = int(_lib.lib.nele_track_stream_record_bytes(tr.Q))
    header = tr.nbytes - tr.S * rec
    return tr.state[header + slot * rec:header + (slot + 1) * rec].clone()


def _status(tr):
    return {k: v.cpu().numpy() for k, v in tr.status().items()}


def feed(tr, mics, playeds, group, slots=None, after=None):
    """all hops of the given streams through ``tr`` (in ``slots``, default 0 ..), ``group`` hops per call at most -> (aligned [n, L] on
    the host, the `moved` masks [calls, S]); after(first hop of the call, hops fed so far, moved): called behind every call"""
    slots = list(range(len(mics))) if slots is None else slots
    L = len(mics[0])
    out, masks = [], []
    for a in range(0, L, group * HOP):
        b = min(L, a + group * HOP)
        D = np.zeros((tr.S, b - a), np.float32)
        X = np.zeros((tr.S, b - a), np.float32)
        act = np.zeros(tr.S, bool)
        for i, s in enumerate(slots):
            D[s], X[s], act[s] = mics[i][a:b], playeds[i][a:b], True
        y, moved = tr.process(torch.from_numpy(D), torch.from_numpy(X), active=None if act.all() else act, want_moved=True)
        out.append(y[slots].cpu().numpy())
        masks.append(moved.cpu().numpy())
        if after is not None:
            after(a // HOP, b // HOP, masks[-1])
    return np.concatenate(out, axis=1), np.array(masks)


def check_status(tag, st, slot, ref, fed, worst):
    """nele_track_status of ``slot`` after ``fed`` hops against the reference's snapshots; worst: [e, conf] largest ratios so far"""
    got = tuple(int(st[k][slot]) for k in INTS)
    assert got == tuple(int(v) for v in ref['ints'][fed - 1]), (tag, fed, got, ref['ints'][fed - 1])
    e, conf = ref['e'][fed - 1], ref['conf'][fed - 1]
    if not e.any():
        assert not st['energies'][slot].any() and st['conf'][slot] == 0.0, (tag, fed)
        return
    scale = float(e.max())
    de = float(np.abs(st['energies'][slot] - e).max() / scale)
    dc = float(abs(st['conf'][slot] - conf))
    worst[0], worst[1] = max(worst[0], de), max(worst[1], dc / scale)
    assert de <= 1e-9, (tag, fed, de)
    assert dc <= 1e-9 * scale and dc <= 1e-9 * abs(conf), (tag, fed, dc, scale, conf)
    assert int(np.argmax(st['energies'][slot])) == int(np.argmax(e))


# -------------------------------------------------------------------------------------------------------- parity against the reference
@pytest.mark.parametrize('B,Q', [(3, 3), (5, 8), (2, 32)])
def test_parity_with_the_reference_through_a_jump(B, Q):
    """every slot of the batch against the reference on its own scenario, 11 hops per call (the last call brings 3), status and `moved`
    compared after every call; (3, 3): the unpaired block, which slots 0 and 1 first lock in"""
    ss = [scen(Q, i) for i in range(B)]
    refs = [ref_run(Q, i) for i in range(B)]
    assert sum(r['ref'].moves == 1 for r in refs) >= 2 and all(r['ref'].moves <= 1 for r in refs)      # there are moves to compare
    tr = _track(B, Q)
    worst = [0.0, 0.0]

    def after(first, fed, moved):
        st = _status(tr)
        for i in range(B):
            tag = 'B %d Q %d slot %d' % (B, Q, i)
            check_status(tag, st, i, refs[i], fed, worst)
            assert moved[i] == int(refs[i]['moved'][first:fed].any()), (tag, first, fed)

    aligned, masks = feed(tr, [s['mic'] for s in ss], [s['played'] for s in ss], 11, after=after)
    assert masks.sum() == sum(r['ref'].moves for r in refs)
    for i in range(B):
        assert np.array_equal(aligned[i], refs[i]['aligned']), i
    assert np.array_equal(tr.delays().cpu().numpy(), [r['ref'].delay for r in refs])
    assert np.array_equal(tr.moves().cpu().numpy(), [r['ref'].moves for r in refs])
    print('B %d Q %d: delays %s, moves %s, worst |e - e_ref| / max e %.3g, worst |conf - conf_ref| / max e %.3g (bound 1e-9)'
          % (B, Q, tr.delays().tolist(), tr.moves().tolist(), worst[0], worst[1]))


def test_parity_with_ragged_active_masks():
    """B = 5, Q = 8: each call brings 6 hops to a random subset of the slots, the others are inactive and their input rows hold NaN - a
    slot that is read while inactive poisons its state; an inactive slot's `moved` is 0"""
    B, Q, G = 5, 8, 6
    ss = [scen(Q, i) for i in range(B)]
    refs = [ref_run(Q, i) for i in range(B)]
    tr = _track(B, Q)
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
        y, moved = tr.process(torch.from_numpy(D), torch.from_numpy(X), active=act, want_moved=True)
        y, moved = y.cpu().numpy(), moved.cpu().numpy()
        for i in range(B):
            if act[i]:
                assert moved[i] == int(refs[i]['moved'][pos[i]:pos[i] + G].any()), (i, pos[i])
                got[i].append(y[i])
                pos[i] += G
            else:
                assert moved[i] == 0
        st = _status(tr)
        for i in range(B):
            if pos[i]:
                check_status('ragged slot %d' % i, st, i, refs[i], int(pos[i]), worst)
    assert list(tr.hops) == [HOPS] * B
    for i in range(B):
        assert np.array_equal(np.concatenate(got[i]), refs[i]['aligned']), i
    print('ragged B 5 Q 8: delays %s, worst |e - e_ref| / max e %.3g, conf %.3g' % (tr.delays().tolist(), worst[0], worst[1]))


# ------------------------------------------------------------------------------------------------- the same search as nele_bulk_hop's
@pytest.mark.parametrize('Q,slot', [(3, 0), (8, 0)])
def test_the_first_search_is_nele_bulk_hop_bit_for_bit(Q, slot):
    """hop by hop, up to and including the hop of the first lock: aligned, delay, e and conf are the bits of BulkDelay on the same input"""
    s = scen(Q, slot)
    lock = ref_run(Q, slot)['ref'].of('lock')[0][0]
    tr, bd = _track(1, Q), _bulk(1, Q)
    for k in range(lock + 1):
        d, x = torch.from_numpy(s['mic'][None, k * HOP:(k + 1) * HOP].copy()), torch.from_numpy(s['played'][None, k * HOP:(k + 1) * HOP].copy())
        assert torch.equal(tr.process(d, x), bd.process(d, x)), k
        st, sb = tr.status(), bd.status()
        assert torch.equal(st['delay'], sb['delay']) and torch.equal(st['energies'], sb['energies']) and torch.equal(st['conf'], sb['conf']), k
    assert st['delay'].item() >= 0 and sb['hops_searched'].item() == lock + 1


@pytest.mark.parametrize('Q,slot', [(3, 0), (8, 0)])
def test_a_background_search_is_a_fresh_search_from_the_hop_behind_its_clear(Q, slot):
    """the search cleared on the hop of the first lock, t0 - 1, against a fresh BulkDelay fed from hop t0: from the background search's
    first evaluated hop up to its `hold` (a confirmation or a give-up cut short by it ends the comparison), e and conf are the same bits"""
    s = scen(Q, slot)
    ev = ref_run(Q, slot)['ref'].events
    t0, until = ev[0][0] + 1, ev[1][0]                                            # the next event: the background search's own end
    assert ev[0][1] == 'lock' and until - t0 + 1 >= Q
    tr, bd = _track(1, Q), _bulk(1, Q)
    tr.process(torch.from_numpy(s['mic'][None, :t0 * HOP].copy()), torch.from_numpy(s['played'][None, :t0 * HOP].copy()))
    assert tr.status()['age'].item() == 0 and tr.delays().item() >= 0
    compared = 0
    for k in range(t0, until + 1):
        d, x = torch.from_numpy(s['mic'][None, k * HOP:(k + 1) * HOP].copy()), torch.from_numpy(s['played'][None, k * HOP:(k + 1) * HOP].copy())
        tr.process(d, x)
        bd.process(d, x)
        st, sb = tr.status(), bd.status()
        if k - t0 + 1 >= Q:                                                       # before: the tracker still reports the hop of the lock
            assert torch.equal(st['energies'], sb['energies']) and torch.equal(st['conf'], sb['conf']), k
            compared += 1
    assert compared >= 2 and sb['hops_searched'].item() == until - t0 + 1
    if ev[1][1] == 'confirm':                                                     # the fresh search locked on the hop on which the tracker confirmed
        assert sb['delay'].item() >= 0 and st['confirms'].item() == 1


# ---------------------------------------------------------------------------------------------------------------- bitwise invariances
def _full_run(tr, s, group, slot=0, others=None):
    """-> (aligned, OR of the calls' moved, status arrays of the slot, its record)"""
    if others is None:
        aligned, masks = feed(tr, [s['mic']], [s['played']], group, slots=[slot])
        aligned = aligned[0]
    else:
        ss = list(others)
        aligned, masks = feed(tr, [x['mic'] for x in ss], [x['played'] for x in ss], group)
        aligned = aligned[slot]
    st = _status(tr)
    return aligned, masks[:, slot].max(), {k: v[slot].copy() for k, v in st.items()}, _record(tr, slot).cpu().numpy()


def _same(a, b):
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    for k in a[2]:
        assert np.array_equal(a[2][k], b[2][k]), k
    assert np.array_equal(a[3], b[3])


@pytest.mark.parametrize('Q', [3, 8])
def test_hop_grouping_and_batch_do_not_change_a_slot(Q):
    """one hop per call = 7 per call (lock and move fall inside calls) = all 300 at once; alone = in slot 3 of B = 5 beside other
    streams: aligned, status and every byte of the record"""
    slot_scen = {3: 1, 8: 3}[Q]
    s = scen(Q, slot_scen)
    r = ref_run(Q, slot_scen)['ref']
    assert r.moves == 1 and r.gaveups >= 1 and r.confirms >= 1
    runs = [_full_run(_track(1, Q), s, group) for group in (1, 7, HOPS)]
    assert runs[0][2]['moves'] == 1 and runs[0][1] == 1 and runs[0][0].any()
    for other in runs[1:]:
        _same(other, runs[0])
    others = [scen(8, i) for i in range(5)]
    others[3] = s
    _same(_full_run(_track(5, Q), s, 5, slot=3, others=others), runs[0])


def test_inactive_slots_are_neither_read_nor_written():
    B, Q, n0, n1 = 3, 8, 60, 6
    ss = [scen(Q, i) for i in range(B)]
    mics, pls = [s['mic'] for s in ss], [s['played'] for s in ss]
    tr = _track(B, Q)
    feed(tr, [m[:n0 * HOP] for m in mics], [p[:n0 * HOP] for p in pls], 12)
    before, st_before = _record(tr, 1), _status(tr)
    # a call that skips slot 1: NaN inputs there, a sentinel-filled output
    D = np.stack([m[n0 * HOP:(n0 + n1) * HOP] for m in mics])
    X = np.stack([p[n0 * HOP:(n0 + n1) * HOP] for p in pls])
    D[1], X[1] = np.nan, np.nan
    out = torch.full((B, n1 * HOP), SENTINEL, device='cuda')
    _, moved = tr.process(torch.from_numpy(D), torch.from_numpy(X), active=[True, False, True], out=out, want_moved=True)
    assert (out[1] == SENTINEL).all() and not (out[0] == SENTINEL).any() and not (out[2] == SENTINEL).any()
    assert moved.tolist() == [0, 0, 0]
    assert torch.equal(_record(tr, 1), before)
    st = _status(tr)
    for k in st:
        assert np.array_equal(st[k][1], st_before[k][1]), k
    # slot 1 goes on where it was: equal to a run that never saw the skipped call
    y1, _ = feed(tr, [mics[1][n0 * HOP:]], [pls[1][n0 * HOP:]], 17, slots=[1])
    alone = _track(1, Q)
    ya, _ = feed(alone, [mics[1]], [pls[1]], HOPS)
    assert np.array_equal(y1[0], ya[0][n0 * HOP:]) and ya.any()
    assert np.array_equal(_record(tr, 1).cpu().numpy(), _record(alone, 0).cpu().numpy())


def test_reset_and_set_delay_touch_one_slot():
    """after 130 hops (every slot locked): reset([1]) leaves a cleared record that runs like a fresh tracker; set_delay([2], 5) leaves
    slot 2 what the reference's set_delay leaves (delay line, counters and hop count kept; the search cleared); slot 0 is as in a run
    without either"""
    B, Q, n0 = 3, 8, 130
    ss = [scen(Q, i) for i in (0, 3, 2)]
    mics, pls = [s['mic'] for s in ss], [s['played'] for s in ss]
    rest = HOPS - n0

    def run(touch):
        tr = _track(B, Q)
        feed(tr, [m[:n0 * HOP] for m in mics], [p[:n0 * HOP] for p in pls], 9)
        if touch:
            assert (tr.delays() >= 0).all()
            tr.reset([1])
            assert tr.delays().tolist()[1] == -1 and not _record(tr, 1).any() and tr.hops[1] == 0
            tr.set_delay([2], 5)
            with pytest.raises(ValueError, match='hops'):
                tr.set_delay([0], Q)
        m2, p2 = [m[n0 * HOP:] for m in mics], [p[n0 * HOP:] for p in pls]
        if touch:
            m2[1], p2[1] = mics[1][:rest * HOP], pls[1][:rest * HOP]
        y, _ = feed(tr, m2, p2, 13)
        return tr, y, [_record(tr, i).cpu().numpy() for i in range(B)]

    tr, y, recs = run(True)
    fresh = _track(1, Q)
    yf, _ = feed(fresh, [mics[1][:rest * HOP]], [pls[1][:rest * HOP]], 41)
    assert np.array_equal(y[1], yf[0]) and yf.any() and np.array_equal(recs[1], _record(fresh, 0).cpu().numpy())
    _, y_, recs_ = run(False)
    assert np.array_equal(y[0], y_[0]) and np.array_equal(recs[0], recs_[0])
    # slot 2 against the reference through the same set_delay
    r = TrackRef(Q, ratio=RATIO, hold=HOLD, patience=PATIENCE)
    r.run(mics[2][:n0 * HOP], pls[2][:n0 * HOP])
    r.set_delay(5)
    want = r.run(mics[2][n0 * HOP:], pls[2][n0 * HOP:])
    st = _status(tr)
    assert np.array_equal(y[2], want) and not np.array_equal(y[2], y_[2])
    assert tuple(int(st[k][2]) for k in INTS) == (r.delay, r.hops, r.age, r.sleep, r.moves, r.confirms, r.gaveups, r.last_move)
    assert st['hops'][2] == HOPS


def test_set_delay_keeps_a_plain_search_state_and_clears_a_trackers():
    """the one place where the two modes of the shared kernels differ on purpose.  B = 2, Q = 3, two searching hops, set_delay([0], 1):
    nele_bulk_set_delay writes the delay and nothing else (hops_searched is still 2, the record apart from that integer is unchanged);
    nele_track_set_delay also clears the search (age 0, awake, a zero search state) and keeps the counters and the hop count"""
    B, Q = 2, 3
    ss = [scen(Q, i) for i in range(B)]
    mic = torch.from_numpy(np.stack([s['mic'][:2 * HOP] for s in ss]))
    played = torch.from_numpy(np.stack([s['played'][:2 * HOP] for s in ss]))
    bd, tr = _bulk(B, Q), _track(B, Q)
    bd.process(mic, played)
    tr.process(mic, played)
    before = {'bulk': _record(bd, 0).cpu().numpy(), 'track': _record(tr, 0).cpu().numpy(), 'st': _status(tr)}
    assert before['st']['age'].tolist() == [2, 2] and np.array_equal(before['bulk'][:24], before['track'][:24]) and before['bulk'][256 + 512:].any()
    bd.set_delay([0], 1)
    tr.set_delay([0], 1)
    st = {k: v.cpu().numpy() for k, v in bd.status().items()}
    assert st['hops_searched'].tolist() == [2, 2] and st['delay'].tolist() == [1, -1]
    rec = _record(bd, 0).cpu().numpy()
    assert np.array_equal(rec[:20], before['bulk'][:20]) and np.array_equal(rec[24:], before['bulk'][24:])      # int [5] is the delay plus one
    st = _status(tr)
    assert (st['age'][0], st['sleep'][0], st['delay'][0], st['hops'][0]) == (0, 0, 1, 2)
    for k in ('moves', 'confirms', 'gaveups', 'last_move'):
        assert st[k][0] == before['st'][k][0], k
    assert all(st[k][1] == before['st'][k][1] for k in INTS) and st['age'][1] == 2
    rec = _record(tr, 0).cpu().numpy()
    line = slice(6144, 6144 + 4 * HOP * Q)                                       # DESIGN.md section 16's record: the delay line is kept,
    assert np.array_equal(rec[line], before['track'][line]) and rec[line].any()  # x_prev, S_d, S_x, the ring and C_q are zero
    assert not rec[256 + 512:line.start].any() and not rec[line.stop:].any()


# ------------------------------------------------------------------------------------------------------------------ rest and patience
def test_rest_skips_the_search_and_keeps_the_output_flowing():
    """rest = 5 at Q = 8, one hop per call: parity with the reference; on every hop that begins with sleep > 0 the search is not run -
    e, conf and age stay as they were, sleep goes down by one - and `aligned` is still `played` of `delay` hops ago"""
    Q, slot, REST = 8, 0, 5
    s = scen(Q, slot)
    ref = ref_run(Q, slot, rest=REST)
    assert ref['ref'].moves == 1
    tr = _track(1, Q, rest=REST)
    worst, slept, prev = [0.0, 0.0], 0, None
    for k in range(HOPS):
        d, x = torch.from_numpy(s['mic'][None, k * HOP:(k + 1) * HOP].copy()), torch.from_numpy(s['played'][None, k * HOP:(k + 1) * HOP].copy())
        y = tr.process(d, x).cpu().numpy()[0]
        st = _status(tr)
        check_status('rest', st, 0, ref, k + 1, worst)
        assert np.array_equal(y, ref['aligned'][k * HOP:(k + 1) * HOP])
        if prev is not None and prev['sleep'][0] > 0:
            slept += 1
            assert st['sleep'][0] == prev['sleep'][0] - 1 and st['age'][0] == prev['age'][0] == 0
            assert np.array_equal(st['energies'], prev['energies']) and np.array_equal(st['conf'], prev['conf'])
            delay = int(st['delay'][0])
            assert delay >= 0 and np.array_equal(y, s['played'][(k - delay) * HOP:(k - delay + 1) * HOP])
        prev = st
    events = len(ref['ref'].events)
    assert slept >= REST * (events - 1) and events >= 4
    print('rest %d: %d hops of %d without search work, %d events' % (REST, slept, HOPS, events))


def test_patience_runs_out_without_an_echo_and_nothing_moves():
    """set_delay(3) on three echo-free microphones at Q = 8 (white noise, the toy noise, the reversed far end), 264 hops, patience 48:
    a give-up every 48 hops, no move, no confirmation, the delay kept; the status as the reference's after every call"""
    B, Q = 3, 8
    neg = [BC.negatives()[i] for i in (0, 8, 16)]
    mics, pls = [n[1] for n in neg], [n[2] for n in neg]
    refs = [ref_of(m, p, Q, set_delay=3) for m, p in zip(mics, pls)]
    tr = _track(B, Q)
    tr.set_delay([0, 1, 2], 3)
    worst = [0.0, 0.0]

    def after(first, fed, moved):
        st = _status(tr)
        for i in range(B):
            check_status('echo-free %d' % i, st, i, refs[i], fed, worst)
        assert not moved.any()

    aligned, _ = feed(tr, mics, pls, 10, after=after)
    st = _status(tr)
    assert st['gaveups'].tolist() == [264 // PATIENCE] * B and not st['moves'].any() and not st['confirms'].any()
    assert st['delay'].tolist() == [3] * B and st['last_move'].tolist() == [-1] * B
    for i in range(B):
        assert np.array_equal(aligned[i], np.concatenate([np.zeros(3 * HOP, np.float32), pls[i]])[:264 * HOP])


# ---------------------------------------------------------------------------------------------------------------------- the composite
def test_tracked_canceller_is_the_chain_by_hand_and_follows_the_jump():
    """B = 2, Q = 32, P = 4, 8 hops per call: TrackedEchoCanceller = TrackingBulkDelay, EchoCanceller.reset_flagged on its device mask,
    EchoCanceller, by hand, bit for bit; its second-half echo reduction is within 0.01 dB of the reference chain's (TrackRef, an AecRef
    begun again at the first hop of the call in which the move fell); the plain AlignedEchoCanceller on the same input stays at the
    reference's untracked figure (BulkRef in front of AecRef)"""
    from nele_gan_amd.aec import EchoCanceller
    from nele_gan_amd.bulkdelay import AlignedEchoCanceller
    from nele_gan_amd.bulktrack import TrackedEchoCanceller
    B, Q, P, G = 2, 32, 4, 8
    ss = [scen(Q, i) for i in range(B)]
    mic = np.stack([s['mic'] for s in ss])
    pl = np.stack([s['played'] for s in ss])
    comp = TrackedEchoCanceller(_track(B, Q), EchoCanceller(B, partitions=P))
    ht, ha = _track(B, Q), EchoCanceller(B, partitions=P)
    plain = AlignedEchoCanceller(_bulk(B, Q), EchoCanceller(B, partitions=P))
    echo, echo_u = [], []
    for a in range(0, HOPS * HOP, G * HOP):
        d, x = torch.from_numpy(mic[:, a:a + G * HOP].copy()).cuda(), torch.from_numpy(pl[:, a:a + G * HOP].copy()).cuda()
        r1, y1 = comp.process(d, x, want_echo=True)
        al, moved = ht.process(d, x, want_moved=True)
        ha.reset_flagged(moved)
        r2, y2 = ha.process(d, al, want_echo=True)
        assert torch.equal(r1, r2) and torch.equal(y1, y2), a
        echo.append(y1.cpu().numpy())
        echo_u.append(plain.process(d, x, want_echo=True)[1].cpu().numpy())
    echo, echo_u = np.concatenate(echo, axis=1).astype(np.float64), np.concatenate(echo_u, axis=1).astype(np.float64)
    assert comp.track.moves().tolist() == [1, 1] and torch.equal(comp.echo_path(), ha.echo_path())
    assert comp.track.delays().tolist() == [ref_run(Q, i)['ref'].delay for i in range(B)]
    # the reference chains on slot 0
    s = ss[0]
    tr_ref, aec_ref, y_ref = TrackRef(Q, ratio=RATIO, hold=HOLD, patience=PATIENCE), AecRef(P), []
    for a in range(0, HOPS * HOP, G * HOP):
        hops = [tr_ref.hop(s['mic'][i:i + HOP], s['played'][i:i + HOP]) for i in range(a, min(a + G * HOP, HOPS * HOP), HOP)]
        if any(h[1] for h in hops):
            aec_ref = AecRef(P)
        y_ref.append(aec_ref.run(s['mic'][a:a + G * HOP], np.concatenate([h[0] for h in hops]))[1])
    _, y_unt = AecRef(P).run(s['mic'], BulkRef(Q, ratio=RATIO, hold=HOLD).run(s['mic'], s['played'])[0])
    red_ref, red_gpu = C.reduction_db(s['echo'], np.concatenate(y_ref)), C.reduction_db(s['echo'], echo[0])
    unt_ref, unt_gpu = C.reduction_db(s['echo'], y_unt), C.reduction_db(s['echo'], echo_u[0])
    print('bulk 5000 -> 1000 at hop %d, ENR 0 dB, hops 150 .. 299: tracked reference %.2f dB, GPU %.2f dB; untracked reference %.2f dB, GPU %.2f dB'
          % (JUMP, red_ref, red_gpu, unt_ref, unt_gpu))
    assert abs(red_gpu - red_ref) <= 0.01
    assert abs(unt_gpu - unt_ref) <= 0.01
    assert red_ref >= unt_ref                                                     # (the reference's own figures; tests/test_track_cpu.py holds them too)


# ----------------------------------------------------------------------------------------------------------------------- command line
def test_command_line(tmp_path, capsys):
    from nele_gan_amd import aec as A
    from nele_gan_amd import dataio
    from nele_gan_amd.bulktrack import TrackedEchoCanceller, TrackingBulkDelay
    Q, P = 32, 3
    s = TC.scenario(5000, 1000, 10.0, 6, 110, 400)
    L = 400 * HOP
    mic_path, pl_path, out_b, out_t = (str(tmp_path / n) for n in ('mic.wav', 'played.wav', 'out_bulk.wav', 'out_track.wav'))
    dataio.write_wav_pcm16(mic_path, s['mic'])
    dataio.write_wav_pcm16(pl_path, s['played'])
    mic, _ = dataio.read_wav(mic_path)
    pl, _ = dataio.read_wav(pl_path)

    def pcm(res):
        return dataio.pcm16_quantise(res).astype(np.float32) / np.float32(32768.0)

    # the composite hop by hop, as the command line runs it
    comp = TrackedEchoCanceller(TrackingBulkDelay(1, blocks=Q), A.EchoCanceller(1, partitions=P))
    res, events, last = [], [], -1
    for k in range(400):
        d, x = torch.from_numpy(mic[None, k * HOP:(k + 1) * HOP].copy()), torch.from_numpy(pl[None, k * HOP:(k + 1) * HOP].copy())
        res.append(comp.process(d, x)[0].cpu().numpy())
        now = comp.track.delays().item()
        if now != last:
            events.append((k, now))
            last = now
    assert len(events) == 2 and comp.track.moves().item() == 1
    assert A.main(['--mic', mic_path, '--played', pl_path, '--out', out_t, '--partitions', str(P), '--bulk-blocks', str(Q), '--bulk-track']) == 0
    said = capsys.readouterr().out
    assert 'bulk delay: locked at hop %d: %d hops' % events[0] in said and 'bulk delay: moved at hop %d: %d hops' % events[1] in said
    out, _ = dataio.read_wav(out_t)
    assert np.array_equal(out[:L], pcm(np.concatenate(res)))
    # without the option: the search that stops at its lock, and not a word about a move
    assert A.main(['--mic', mic_path, '--played', pl_path, '--out', out_b, '--partitions', str(P), '--bulk-blocks', str(Q)]) == 0
    said = capsys.readouterr().out
    assert 'moved' not in said and 'locked' not in said and 'bulk delay: %d hops' % events[0][1] in said
    out2, _ = dataio.read_wav(out_b)
    assert not np.array_equal(out2, out)
    # an echo-free microphone: none found; the option needs --bulk-blocks
    far, _ = C.far_and_near()
    dataio.write_wav_pcm16(mic_path, far[::-1].astype(np.float32))
    dataio.write_wav_pcm16(pl_path, far.astype(np.float32))
    assert A.main(['--mic', mic_path, '--played', pl_path, '--out', out_t, '--bulk-blocks', '8', '--bulk-track']) == 0
    assert 'bulk delay: none found in 8 blocks' in capsys.readouterr().out
    with pytest.raises(SystemExit):
        A.main(['--mic', mic_path, '--played', pl_path, '--out', out_t, '--bulk-track'])
