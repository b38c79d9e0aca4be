"""GPU: the running ESTOI (nele_gan_amd/monitor.py, csrc/monitor.hip) against tests/monitor_ref.py, the float64 numpy statement of
DESIGN.md section 27 that tests/test_monitor_cpu.py ties to oracle/estoi.py.  Counts and gate decisions are compared exactly (no frame
of a case lies within estoi_cases.GATE_MARGIN_DB of the gate), the loudest frame within the project's 1e-9 dB, every segment value,
the last and the smoothed reading within DSEG_ABS = 1e-9 and the sum within count x DSEG_ABS.  Then the streaming contract, bit for
bit: hop grouping, batch and slot, inactive neighbours, reset, lag, the implied deg; and MonitoredEnhancer around the rule-mode enhancer
and the limited, compressed chain.

Measured on an MI355X: over the eight cases and the five-stream launch every d is within 1.2e-14 of the reference, M within 3.6e-15 dB,
the sum within 2.4e-14, the smoothed reading within 4.7e-16, and every count is equal; the whole file runs in 4 s."""
import numpy as np
import pytest

import estoi_cases as EC
import monitor_cases as C
import monitor_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

HOP = R.HOP
DSEG_ABS = 1e-9                  # a segment value (tests/test_estoi_stages_gpu.py)
EN_DB = 1e-9                     # a frame energy in dB (the same)
WANT = ('stats', 'seg', 'nseg')
EXACT = (R.COUNT, R.SKIPPED, R.SEEN, R.KEPT)


def _mon(B, lag=0, tc=0.25):
    from nele_gan_amd.monitor import StreamMonitor
    return StreamMonitor(B, lag=lag, time_constant=tc)


def feed(mon, refs, degs, adds=None, group=5, slots=None, start=0, stop=None, fill=None):
    """hops start .. stop of the given streams through ``mon`` (in ``slots``, default 0 ..), ``group`` hops per call at most; the other
    slots inactive (fill None: their columns hold NaN) or active on ``fill(shape)`` -> dict: seg [n, nh, 2], nseg [n, nh], stats [n, 8]
    after the last call, on the host.  degs / adds: lists, or None."""
    slots = list(range(len(refs))) if slots is None else slots
    L = len(refs[0]) if stop is None else stop * HOP
    parts = {'seg': [], 'nseg': []}
    stats = None
    for a in range(start * HOP, L, group * HOP):
        b = min(L, a + group * HOP)
        act = np.zeros(mon.S, bool)
        sig = []
        for src in (refs, degs, adds):
            if src is None:
                sig.append(None)
                continue
            X = np.full((mon.S, b - a), np.nan, np.float32) if fill is None else fill((mon.S, b - a))
            for i, s in enumerate(slots):
                X[s], act[s] = src[i][a:b], True
            sig.append(torch.from_numpy(X))
        if fill is not None:
            act[:] = True
        st, seg, nseg = mon.process(sig[0], sig[1], sig[2], active=None if act.all() else act, want=WANT)
        parts['seg'].append(seg[slots].cpu().numpy())
        parts['nseg'].append(nseg[slots].cpu().numpy())
        stats = st[slots].cpu().numpy()
    return {'seg': np.concatenate(parts['seg'], axis=1), 'nseg': np.concatenate(parts['nseg'], axis=1), 'stats': stats}


def bits(a):
    return np.ascontiguousarray(a).view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def same(a, b, row_a=slice(None), row_b=slice(None)):
    return all(a[k][row_a].shape == b[k][row_b].shape and np.array_equal(bits(a[k][row_a]), bits(b[k][row_b])) for k in ('seg', 'nseg', 'stats'))


def records(mon, slots):
    """the slots' state records, byte for byte"""
    from nele_gan_amd._lib import lib
    rec = lib.nele_mon_stream_record_bytes()
    return mon.state[mon.nbytes - mon.S * rec:].reshape(mon.S, rec)[slots].cpu().numpy()


def check_parity(tag, got, row, ref):
    seg, nseg, s, r = got['seg'][row], got['nseg'][row], got['stats'][row], ref['stats']
    both = ~np.isnan(ref['seg'])
    worst = float(np.max(np.abs(seg[both] - ref['seg'][both]))) if both.any() else 0.0
    print('%s: %d segments counted, %d skipped, %d of %d frames kept; max |d - ref| %.3g, |M - ref| %.3g dB, |sum - ref| %.3g, |smoothed - ref| %.3g'
          % (tag, s[R.COUNT], s[R.SKIPPED], s[R.KEPT], s[R.SEEN], worst, abs(s[R.M] - r[R.M]), abs(s[R.SUM] - r[R.SUM]), abs(s[R.SMOOTH] - r[R.SMOOTH])))
    assert seg.dtype == np.float64 and nseg.dtype == np.int32 and s.dtype == np.float64 and not np.isnan(s).any()
    assert np.array_equal(nseg, ref['nseg'])
    for k in EXACT:
        assert s[k] == r[k], (tag, k)
    assert abs(s[R.M] - r[R.M]) <= EN_DB
    assert np.array_equal(np.isnan(seg), np.isnan(ref['seg'])) and worst <= DSEG_ABS
    assert abs(s[R.LAST] - r[R.LAST]) <= DSEG_ABS and abs(s[R.SMOOTH] - r[R.SMOOTH]) <= DSEG_ABS
    assert abs(s[R.SUM] - r[R.SUM]) <= max(r[R.COUNT], 1) * DSEG_ABS


# -------------------------------------------------------------------------------------------------------- parity against the reference
@pytest.mark.parametrize('name', C.NAMES)
def test_parity_with_the_reference(name):
    """every case alone in a state of one slot, 5 hops per call"""
    x, y = C.case(name)
    check_parity(name, feed(_mon(1), [x], [y]), 0, C.reference(name))


def test_parity_of_five_cases_in_one_launch_with_an_added_signal_and_a_lag():
    """B = 5, 40 hops, lag 2, 7 hops per call: the first 40 hops of five cases side by side, deg two hops late, a third signal summed
    onto it"""
    names = ('steady', 'gapped', 'quiet_start', 'silence', 'nan_deg')
    xs = [C.case(n)[0][:40 * HOP] for n in names]
    ys = [np.concatenate([np.zeros(2 * HOP, np.float32), C.case(n)[1][:38 * HOP]]) for n in names]
    add = (0.01 * np.random.default_rng(3).standard_normal(40 * HOP)).astype(np.float32)
    got = feed(_mon(5, lag=2), xs, ys, [add] * 5, group=7)
    for i, n in enumerate(names):
        check_parity('%s + add, lag 2' % n, got, i, R.run(xs[i], ys[i], add, lag=2, alpha=C.ALPHA))
    assert got['stats'][0][R.COUNT] > 0 and got['stats'][3][R.SKIPPED] > 0


# ------------------------------------------------------------------------------------------------------------ the streaming contract
def test_bits_do_not_depend_on_the_hop_grouping():
    """quiet_start, 72 hops: one hop per call, 3, 7 and all at once - outputs and the state record, bit for bit"""
    x, y = C.case('quiet_start')
    runs = []
    for group in (1, 3, 7, 72):
        mon = _mon(1, lag=1)
        runs.append((feed(mon, [x], [y], group=group), records(mon, [0])))
    for got, rec in runs[1:]:
        assert same(got, runs[0][0]) and np.array_equal(rec, runs[0][1])
    assert runs[0][0]['stats'][0][R.COUNT] > 20


def test_bits_do_not_depend_on_the_batch_the_slot_or_the_neighbours():
    """the same stream alone (B = 1), in slot 129 of 130 beside 129 active slots on other noise, and beside 129 inactive ones"""
    x, y = C.case('quiet_start')
    alone_mon = _mon(1)
    alone = feed(alone_mon, [x], [y], group=9)
    rng = np.random.default_rng(8)
    busy_mon, idle_mon = _mon(130), _mon(130)
    busy = feed(busy_mon, [x], [y], group=9, slots=[129], fill=lambda shape: (0.05 * rng.standard_normal(shape)).astype(np.float32))
    idle = feed(idle_mon, [x], [y], group=9, slots=[129])
    assert same(busy, alone) and same(idle, alone)
    assert np.array_equal(records(busy_mon, [129]), records(alone_mon, [0])) and np.array_equal(records(idle_mon, [129]), records(alone_mon, [0]))
    assert not records(idle_mon, [0, 77, 128]).any()                              # an inactive slot is not written
    assert busy_mon.read().stats[5, R.SEEN].item() == alone['stats'][0][R.SEEN]   # the neighbours ran


def test_reset_restarts_one_slot_and_leaves_its_neighbours():
    """three slots, 72 hops; slot 1 (steady noise) is reset after 30: its neighbours' bits are those of an undisturbed run, its own
    those of a fresh stream on the remaining 42 hops"""
    x, y = C.case('quiet_start')
    u, v = (a[:len(x)] for a in C.case('nan_both'))
    xs, ys = [x, u, x], [y, v, y]
    mon = _mon(3)
    first = feed(mon, xs, ys, stop=30)
    mon.reset([1])
    assert mon.read().stats[1].cpu().numpy().tolist() == [0, 0, 0, 0, 0, 0, 0, -np.inf] and mon.hops.tolist() == [30, 0, 30]
    rest = feed(mon, xs, ys, start=30)
    whole = feed(_mon(3), xs, ys)
    for s in (0, 2):
        assert np.array_equal(bits(np.concatenate([first['seg'][s], rest['seg'][s]])), bits(whole['seg'][s]))
        assert np.array_equal(bits(rest['stats'][s]), bits(whole['stats'][s]))
    fresh = feed(_mon(1), [xs[1][30 * HOP:]], [ys[1][30 * HOP:]])
    assert same(rest, fresh, row_a=slice(1, 2)) and fresh['stats'][0][R.COUNT] > 0


@pytest.mark.parametrize('lag', [1, 2, 3, 4])
def test_a_lag_is_ref_shifted_early(lag):
    """deg and add of hop h against ref of hop h - lag: the bits of lag 0 on (ref[:-lag hops], deg[lag hops:], add[lag hops:]), and
    nothing in the first lag hops"""
    x, y = C.case('quiet_start')
    add = (0.01 * np.random.default_rng(4).standard_normal(len(x))).astype(np.float32)
    got = feed(_mon(1, lag=lag), [x], [y], [add], group=5)
    zero = feed(_mon(1), [x[:-lag * HOP]], [y[lag * HOP:]], [add[lag * HOP:]], group=5)
    assert not got['nseg'][0][:lag].any() and np.isnan(got['seg'][0][:lag]).all()
    assert np.array_equal(bits(got['seg'][0][lag:]), bits(zero['seg'][0])) and np.array_equal(got['nseg'][0][lag:], zero['nseg'][0])
    assert np.array_equal(bits(got['stats']), bits(zero['stats'])) and zero['stats'][0][R.COUNT] > 20


def test_no_deg_means_the_delayed_ref():
    """deg = None with add: the unprocessed baseline, the bits of deg = ref delayed by lag hops passed explicitly"""
    x, _ = C.case('quiet_start')
    add = (0.02 * np.random.default_rng(6).standard_normal(len(x))).astype(np.float32)
    late = np.concatenate([np.zeros(2 * HOP, np.float32), x[:-2 * HOP]])
    implied = feed(_mon(1, lag=2), [x], None, [add])
    explicit = feed(_mon(1, lag=2), [x], [late], [add])
    assert same(implied, explicit) and implied['stats'][0][R.COUNT] > 20 and 0.05 < implied['stats'][0][R.SUM] / implied['stats'][0][R.COUNT] < 0.95
    clean = feed(_mon(1, lag=2), [x], None, None)                                  # and without add the signal against itself: d = 1
    assert np.nanmin(clean['seg']) > 1 - 1e-9


def test_process_returns_nothing_by_default_and_read_maps():
    from nele_gan_amd.monitor import map_estoi
    x, y = C.case('steady')
    mon = _mon(2)
    X, Y = torch.from_numpy(np.stack([x, x])), torch.from_numpy(np.stack([y, x]))
    assert mon.process(X, Y) is None and mon.hops.tolist() == [40, 40]
    r, m = mon.read(), mon.read(mapped=True)
    ref = C.reference('steady')['stats']
    assert tuple(r.stats.shape) == (2, 8) and r.stats.is_cuda and r.stats.dtype == torch.float64
    assert abs(r.estoi[0].item() - ref[R.SUM] / ref[R.COUNT]) <= DSEG_ABS and r.segments[0].item() == ref[R.COUNT] and r.skipped[0].item() == 0
    assert abs(r.estoi[1].item() - 1.0) < 1e-9 and abs(r.last[0].item() - ref[R.LAST]) <= DSEG_ABS
    assert torch.equal(m.estoi, map_estoi(r.estoi)) and torch.equal(m.smoothed, map_estoi(r.smoothed)) and torch.equal(m.segments, r.segments)
    seg, = mon.process(X[:, :HOP], Y[:, :HOP], want='seg')
    assert tuple(seg.shape) == (2, 1, 2)
    with pytest.raises(ValueError):
        mon.process(X[:, :100], Y[:, :100])
    with pytest.raises(ValueError):
        mon.process(X, Y, want=('gain',))
    with pytest.raises(ValueError):
        mon.process(X, Y[:, :HOP])


# ------------------------------------------------------------------------------------------------------------ beside the enhancer
def _inner(kind, B):
    from nele_gan_amd.drc import CompressedEnhancer, StreamCompressor
    from nele_gan_amd.limiter import LimitedEnhancer, StreamLimiter
    from nele_gan_amd.realtime import RealtimeEnhancer
    from nele_gan_amd.siiopt import SiiOptRule
    rt = RealtimeEnhancer(rule=SiiOptRule(), streams=B)
    return rt if kind == 'rule' else LimitedEnhancer(CompressedEnhancer(rt, StreamCompressor(B)), StreamLimiter(B))


@pytest.mark.parametrize('kind,lag', [('rule', 1), ('limited', 3)])
def test_the_monitored_enhancer_returns_the_inner_output_and_measures_it(kind, lag):
    """(B, hops) = (2, 60), 6 hops per call: the output is the bare inner object's bit for bit; the monitor's readings are the
    reference's on (clean delayed, out + noise), the baseline's on (clean delayed, clean delayed + noise), benefit() their difference"""
    from nele_gan_amd import synth
    from nele_gan_amd.monitor import MonitoredEnhancer, StreamMonitor
    B, nh = 2, 60
    clean, noise = synth.batch(B, nh * HOP, start=40)
    chain = MonitoredEnhancer(_inner(kind, B), StreamMonitor(B, lag=lag, time_constant=0.25), StreamMonitor(B, lag=lag, time_constant=0.25))
    bare = _inner(kind, B)
    assert chain.lag_hops == lag
    outs = []
    for a in range(0, nh * HOP, 6 * HOP):
        c, n = torch.from_numpy(clean[:, a:a + 6 * HOP].copy()), torch.from_numpy(noise[:, a:a + 6 * HOP].copy())
        out = chain.process(c, n)
        assert torch.equal(out, bare.process(c.cuda(), n.cuda()))
        outs.append(out.cpu().numpy())
    out = np.concatenate(outs, axis=1)
    got, base, benefit = chain.mon.read().stats.cpu().numpy(), chain.baseline.read().stats.cpu().numpy(), chain.benefit().cpu().numpy()
    for b in range(B):
        ref = R.run(clean[b], out[b], noise[b], lag=lag, alpha=C.ALPHA)
        raw = R.run(clean[b], None, noise[b], lag=lag, alpha=C.ALPHA)
        assert C.margin(ref['frames']) > EC.GATE_MARGIN_DB and ref['stats'][R.COUNT] > 0
        for s, r in ((got[b], ref['stats']), (base[b], raw['stats'])):
            for k in EXACT:
                assert s[k] == r[k], (b, k)
            assert abs(s[R.M] - r[R.M]) <= EN_DB and abs(s[R.LAST] - r[R.LAST]) <= DSEG_ABS and abs(s[R.SMOOTH] - r[R.SMOOTH]) <= DSEG_ABS
            assert abs(s[R.SUM] - r[R.SUM]) <= r[R.COUNT] * DSEG_ABS
        print('%s stream %d: ESTOI processed %.4f, unprocessed %.4f over %d segments; benefit() %.4f'
              % (kind, b, got[b][R.SUM] / got[b][R.COUNT], base[b][R.SUM] / base[b][R.COUNT], got[b][R.COUNT], benefit[b]))
        assert benefit[b] == got[b][R.SMOOTH] - base[b][R.SMOOTH]
    chain.reset([0])
    assert chain.mon.read().segments.cpu().numpy().tolist() == [0, got[1][R.COUNT]] and chain.baseline.read().segments[0].item() == 0
