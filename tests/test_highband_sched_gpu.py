"""GPU: the up-converter on a hop schedule that carries the band above 8 kHz (nele_gan_amd/highband.py ScheduledHighBandUp,
csrc/highband_sched.hip) and FullBandScheduledEnhancer / adapt_fullband (nele_gan_amd/streamrate.py) against DESIGN.md section 25: the
composition built from the existing scheduled converter and float32 torch ops on the host (bitwise for g = 1, 0.5, 0),
tests/highband_sched_ref.py with the specification's float32 roundings (g = 0.7), the identity, the streaming contract (grouping, batch,
slots, reset: bitwise), HighBandUp at 48 kHz (bitwise), the guard on the lead, the wrapper against the chain built by hand (bitwise), an
18 kHz tone through the whole wrapper at 44.1 kHz, and an impulse.

The composition.  gcd(up, down) = 1, so there are a, b >= 0 with a down - b up = -s (highband_sched_ref.solve_ab): the converter from
the lead L0 - s gives, as output m, the same K products in the same order as output m + a of ScheduledStreamResampler(16 kHz -> rate)
fed b zeros in front of d.
Bounds.  Composition: equal bits - g low and g x are exact products for g = 1, 0.5, 0, so fmaf(-g, low, enh) and fmaf(g, x, u) are the
correctly rounded difference and sum torch computes.  g = 0.7: resample_ref.bound per sample (one float32 ulp of the result plus 1e-12
max |d|, the converter's own bound) plus one float32 ulp of g x: section 24's.  The guard's runs, whose reference
(highband_sched_ref.direct) sums in another order: that plus one float32 ulp of u - the order may move (float)u across a rounding
boundary, and y moves with it.  Tone: 1e-5, section 24's (18 kHz is 1.96 x above the stop-band edge of 1.15 x 8 kHz; the float64 reference gives the gain within 3e-14:
tests/test_highband_sched_cpu.py).
Measured on an MI355X: bit-equal to the composition in all 18 cases (6 cases, 3 gains); g = 0.7: largest |gpu - reference| / bound 0.000
in all six cases and in the guard's three calls off the schedule (every sample bit-equal to the reference); 18 kHz tone in phase
0.999998930 / 0.999998996 with the band (quadrature <= 7.8e-7), 0.499998931 / 0.499998997 at gain 0.5, 1.5e-6 / 1.4e-6 left without
it; impulse peaks exactly ``latency`` late (1005 -> 1888, 1510 -> 2393; lag_hops 2: 1005 -> 2594, 1510 -> 3099); the whole file runs in
3.5 s."""
import numpy as np
import pytest

import highband_sched_ref as HS
import resample_ref as R
import schedrate_ref as S
from highband_ref import fma32

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from weights_recipe import seeded_state_arrays  # noqa: E402

B, HOPS, GROUPS, SENTINEL, START2 = 3, 7, (3, 4), -7.25, 2
# 88.2 kHz with lag_hops 3: a record of 5420 floats, above the 4096 the staging space holds - it moves in two chunks
CASES = [(44100, 'high', 1), (44100, 'high', 2), (22050, 'high', 1), (88200, 'high', 1), (44100, 'scipy', 1), (88200, 'high', 3)]
_RUNS = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _hb(streams, rate, quality='high', lag_hops=1, g=None):
    from nele_gan_amd.highband import ScheduledHighBandUp
    hb = ScheduledHighBandUp(streams, rate, lag_hops, quality)
    if g is not None:
        hb.gain.fill_(g)
    return hb


def _signals(hb, starts, seed, hops=HOPS):
    """one (enh, low, x) per schedule position of ``starts``: float32 Gaussian rows without a zero sample, hops * 256 samples of enh and
    low and the schedule's width of x from there; row 1 scaled by 1e-6 and row 2 by 1e3"""
    rs = np.random.RandomState(seed)
    rows = []
    for k, start in enumerate(starts):
        scale = np.float32({1: 1e-6, 2: 1e3}.get(k, 1.0))
        row = []
        for width in (hops * S.HOP, hops * S.HOP, hb.width_out(hops, start)):
            v = rs.randn(width).astype(np.float32)
            v[v == 0.0] = 1.0
            row.append(v * scale)
        rows.append(tuple(row))
    return rows


def _delayed(v, n):
    """v behind n zeros, cut to v's length, along the last axis (numpy or torch)"""
    if isinstance(v, np.ndarray):
        return np.concatenate([np.zeros(v.shape[:-1] + (n,), v.dtype), v], axis=-1)[..., :v.shape[-1]]
    return torch.cat([torch.zeros(tuple(v.shape[:-1]) + (n,), dtype=v.dtype), v], dim=-1)[..., :v.shape[-1]]


def feed(hb, rows, groups, slots=None, out=False):
    """the signals ``rows`` (one (enh, low, x) per slot of ``slots``, default all; those slots stand at one position) through ``hb``,
    ``groups`` hops per call in turn -> one output row per slot, on the host"""
    slots = list(range(hb.S)) if slots is None else slots
    active = None if len(slots) == hb.S else [s in slots for s in range(hb.S)]
    ys, h, at = [], 0, 0
    for g in groups:
        pos = int(hb.positions[slots[0]])
        w = hb.width_out(g, pos)
        E, Lo, X = (np.zeros((hb.S, n), dtype=np.float32) for n in (g * S.HOP, g * S.HOP, w))
        for k, s in enumerate(slots):
            E[s], Lo[s], X[s] = rows[k][0][h * S.HOP:(h + g) * S.HOP], rows[k][1][h * S.HOP:(h + g) * S.HOP], rows[k][2][at:at + w]
        buf = torch.full((hb.S, w), SENTINEL, device='cuda') if out else None
        y = hb.process(torch.from_numpy(E).cuda(), torch.from_numpy(Lo).cuda(), torch.from_numpy(X).cuda(), active=active, out=buf)
        assert (buf is None or y is buf) and y.shape == (hb.S, w)
        ys.append(y.cpu().numpy()[slots])
        h, at = h + g, at + w
    assert all(at == len(r[2]) for r in rows)
    return list(np.concatenate(ys, axis=1))


def run(rate, quality, lag_hops, g=1.0):
    """(rows, ys) of the case: slots 0 and 1 from position 0 and slot 2, reset to position START2, from there in calls of its own, each
    HOPS hops in calls of GROUPS: one GPU run, shared, never changed"""
    key = (rate, quality, lag_hops, g)
    if key not in _RUNS:
        hb = _hb(B, rate, quality, lag_hops, g)
        assert hb.period in (5, 10) and hb.position == 0
        hb.reset([2], position=START2)
        assert hb.positions.tolist() == [0, 0, START2]
        rows = _signals(hb, (0, 0, START2), rate // 100 + lag_hops + len(quality))
        y01 = feed(hb, rows[:2], GROUPS, slots=[0, 1])
        assert hb.positions.tolist() == [HOPS % hb.period, HOPS % hb.period, START2]
        y2 = feed(hb, rows[2:], GROUPS, slots=[2])
        assert hb.hops.tolist() == [HOPS] * B and hb.positions[2] == (START2 + HOPS) % hb.period
        _RUNS[key] = (rows, y01 + y2)
    return _RUNS[key]


def composed_u(rate, quality, shift, d):
    """ScheduledStreamResampler(16 kHz -> rate) on b zeros + d (+ zeros up to whole hops), from output a on: torch [rows, ..] on the host"""
    from nele_gan_amd.resample import ScheduledStreamResampler
    up = ScheduledStreamResampler(d.shape[0], S.RATE, rate, quality)
    a, b = HS.solve_ab(up.up, up.down, shift)
    hops = d.shape[1] // S.HOP + 2                           # b < down <= 2 hops of input; a < up <= 2 hops of output
    fed = torch.zeros((d.shape[0], hops * S.HOP), dtype=torch.float32)
    fed[:, b:b + d.shape[1]] = d
    return up.process(fed).cpu()[:, a:]


def composed(rate, quality, lag_hops, g, rows):
    """composed_u(enh - g low delayed) + g x delayed: subtraction, delays and addition in float32 torch on the host -> one numpy row each"""
    from nele_gan_amd.highband import highband_sched_plan
    plan = highband_sched_plan(rate, lag_hops, quality)
    gt = torch.tensor(g, dtype=torch.float32)
    e, lo = (torch.from_numpy(np.stack([r[k] for r in rows])) for k in (0, 1))
    u = composed_u(rate, quality, plan['shift'], e - gt * _delayed(lo, plan['lag16']))
    out = []
    for k, r in enumerate(rows):
        y = u[k, :len(r[2])] + gt * _delayed(torch.from_numpy(r[2]), plan['lag'])
        assert y.dtype == torch.float32 and len(y) == len(r[2])
        out.append(y.numpy())
    return out


# ------------------------------------------------------------------------------------------------- 1. the composition
@pytest.mark.parametrize('rate,quality,lag_hops', CASES)
def test_bit_identical_to_the_composition_for_exact_gains(rate, quality, lag_hops):
    for g in (1.0, 0.5, 0.0):
        rows, ys = run(rate, quality, lag_hops, g)
        want = composed(rate, quality, lag_hops, g, rows)
        for b in range(B):
            assert ys[b].shape == want[b].shape == rows[b][2].shape
            assert np.array_equal(_bits(ys[b]), _bits(want[b])), (g, b)
    assert not np.array_equal(run(rate, quality, lag_hops, 1.0)[1][0], run(rate, quality, lag_hops, 0.5)[1][0])


def _lib_taps(hb):
    from nele_gan_amd.resample import taps
    return taps(hb.up, hb.down, hb.zeros, hb.beta, layout=0)


def _bound(y64, d, gx):
    """resample_ref.bound with the largest |d| plus one float32 ulp of g x"""
    return R.bound(y64, float(np.abs(d).max())) + np.spacing(np.abs(gx.astype(np.float32))).astype(np.float64)


@pytest.mark.parametrize('rate,quality,lag_hops', CASES)
def test_an_inexact_gain_against_the_reference(rate, quality, lag_hops):
    g = 0.7
    rows, ys = run(rate, quality, lag_hops, g)
    g32 = np.float32(g)
    h = _lib_taps(_hb(1, rate, quality, lag_hops))
    worst = 0.0
    for b, start in enumerate((0, 0, START2)):
        enh, low, x = rows[b]
        ref = HS.HighBandSchedRef(rate, lag_hops, quality, g=g, rounded=True, pos=start, taps=h)
        y64 = ref.process(enh, low, x)
        d = enh.astype(np.float64) - float(g32) * _delayed(low, ref.lam)
        worst = max(worst, float((np.abs(ys[b].astype(np.float64) - y64) / _bound(y64, d, g32 * _delayed(x, ref.Lx))).max()))
    print('%d Hz %s, lag_hops %d, g = 0.7: largest |gpu - reference| / bound = %.3f' % (rate, quality, lag_hops, worst))
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------- 2. the identity
@pytest.mark.parametrize('rate,quality,lag_hops', CASES)
def test_an_enhancer_that_changes_nothing_gives_the_bits_of_the_input_delayed_by_Lx(rate, quality, lag_hops):
    hb = _hb(B, rate, quality, lag_hops)
    rows = [(_delayed(low, hb.lag16), low, x) for _, low, x in _signals(hb, (0, 0, 0), 5)]
    ys = feed(hb, rows, (1,) * HOPS)
    for b in range(B):
        assert np.array_equal(_bits(ys[b]), _bits(_delayed(rows[b][2], hb.lag)))
        assert not (rows[b][2] == 0.0).any()
    assert hb.lag > hb.hop_max                               # x[m - Lx] reaches two hops back


# ------------------------------------------------------------------------------------------------- 3. grouping and batch
@pytest.mark.parametrize('rate,quality,lag_hops', CASES)
def test_hop_grouping_batch_and_out_buffer_do_not_change_a_slot(rate, quality, lag_hops):
    rows, ys = run(rate, quality, lag_hops)                  # calls of (3, 4) hops
    for groups, out in (((1,) * HOPS, False), ((4, 3), True)):
        hb = _hb(B, rate, quality, lag_hops)
        got = feed(hb, rows[:2], groups, slots=[0, 1], out=out)
        assert np.array_equal(got[0], ys[0]) and np.array_equal(got[1], ys[1]), groups
    alone = _hb(1, rate, quality, lag_hops)
    alone.reset([0], position=START2)
    assert np.array_equal(feed(alone, rows[2:], (5, 2))[0], ys[2])
    five = _hb(5, rate, quality, lag_hops)
    five.reset(range(5), position=START2)
    others = _signals(five, (START2,) * 5, 11)[::-1]
    others[2] = rows[2]
    assert np.array_equal(feed(five, others, (1, 6))[2], ys[2])


def test_rows_of_wider_tensors_pass_without_a_copy():
    """low as rows 0 .. B - 1 of a [2 B, ..] tensor, x likewise, enh with a stride of its own"""
    rows, ys = run(44100, 'high', 1)
    hb = _hb(2, 44100)
    n16, w = HOPS * S.HOP, hb.width_out(HOPS, 0)
    both16 = torch.full((4, n16), float('nan'), device='cuda')
    both44 = torch.full((4, w), float('nan'), device='cuda')
    wide = torch.full((2, n16 + 64), float('nan'), device='cuda')
    for b in range(2):
        wide[b, :n16], both16[b], both44[b] = (torch.from_numpy(v).cuda() for v in rows[b])
    got = hb.process(wide[:, :n16], both16[:2], both44[:2]).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(np.stack(ys[:2])))
    with pytest.raises(ValueError, match='low16 must be'):
        hb.process(wide[:, :n16], torch.zeros((n16, 2), device='cuda').t(), both44[:2])       # the shape, but columns 2 apart
    with pytest.raises(ValueError, match='x_dev must be'):
        hb.process(wide[:, :n16], both16[:2], both44[:2, :w - 1])                            # not the schedule's width of 7 hops
    with pytest.raises(ValueError, match='x_dev must be'):
        hb.process(wide[:, :n16], both16[:2], both44[:2].cpu())
    with pytest.raises(ValueError, match='out must be'):
        hb.process(wide[:, :n16], both16[:2], both44[:2, :hb.width_out(HOPS)], out=torch.zeros((2, 7), device='cuda'))
    hb.positions[1] = 3
    with pytest.raises(ValueError, match='stand at schedule positions'):
        hb.process(wide[:, :n16], both16[:2], both44[:2, :hb.width_out(HOPS)])
    assert (hb.hops == HOPS).all() and hb.position == HOPS % 5


# ------------------------------------------------------------------------------------------------- 4. HighBandUp at the whole-hop rates
@pytest.mark.parametrize('lag_hops', [1, 2])
def test_at_48_khz_it_is_highbandup_bit_for_bit(lag_hops):
    from nele_gan_amd.highband import HighBandUp
    new, old = _hb(B, 48000, 'high', lag_hops, 0.7), HighBandUp(B, 48000, lag_hops)
    old.gain.fill_(0.7)
    assert (new.shift, new.period, new.lag, new.lag16, new.H) == (0, 1, old.lag, old.lag16, old.K - 1) and new.width_out(3) == 3 * old.hop_out
    enh, low, x = (torch.from_numpy(np.stack([r[k] for r in _signals(new, (0, 0, 0), 48, hops=5)])).cuda() for k in range(3))
    a = torch.cat([new.process(enh[:, :512], low[:, :512], x[:, :1536]), new.process(enh[:, 512:], low[:, 512:], x[:, 1536:])], dim=1)
    b = torch.cat([old.process(enh[:, :512], low[:, :512], x[:, :1536]), old.process(enh[:, 512:], low[:, 512:], x[:, 1536:])], dim=1)
    assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy())) and torch.isfinite(a).all() and a.abs().max() > 0


# ------------------------------------------------------------------------------------------------- 5. slots
def _record(hb, slot):
    from nele_gan_amd import _lib
    rec = int(_lib.lib.nele_hbsched_record_bytes(hb.H, hb.lag16, hb.lag))
    header = hb.nbytes - hb.S * rec
    assert header == 256 and rec == HS.record_bytes(hb.H, hb.lag16, hb.lag)
    return hb.state[header + slot * rec:header + (slot + 1) * rec].clone()


def _lead(record):
    return int(record[:4].cpu().numpy().view(np.int32)[0])


@pytest.mark.parametrize('rate,quality,lag_hops', [(44100, 'high', 1), (22050, 'high', 1), (88200, 'high', 3)])
def test_inactive_slots_are_neither_read_nor_written(rate, quality, lag_hops):
    rows, ys = run(rate, quality, lag_hops)
    hb = _hb(B, rate, quality, lag_hops)
    n0, n1 = 2, hb.period                                    # slot 1 sits out one period: it is in step again afterwards
    w0, w1 = hb.width_out(n0, 0), hb.width_out(n1, n0)
    cut = lambda r, h0, h1, a0, a1: (r[0][h0 * S.HOP:h1 * S.HOP], r[1][h0 * S.HOP:h1 * S.HOP], r[2][a0:a1])
    long_rows = _signals(hb, (0, 0), 3, hops=n0 + n1 + 1)
    feed(hb, [cut(r, 0, n0, 0, w0) for r in long_rows], (n0,), slots=[0, 1])
    before = _record(hb, 1)
    assert before.any() and _lead(before) == HS.plan(rate, lag_hops, quality)['L0'] + n0 * S.HOP * -hb.up + w0 * hb.down
    E, Lo, X = (torch.full((B, n), float('nan'), device='cuda') for n in (n1 * S.HOP, n1 * S.HOP, w1))
    part = cut(long_rows[0], n0, n0 + n1, w0, w0 + w1)
    E[0], Lo[0], X[0] = (torch.from_numpy(v).cuda() for v in part)
    out = torch.full((B, w1), SENTINEL, device='cuda')
    hb.process(E, Lo, X, active=[True, False, False], out=out)
    assert (out[1:] == SENTINEL).all() and torch.isfinite(out[0]).all() and not (out[0] == SENTINEL).any()
    assert torch.equal(_record(hb, 1), before) and hb.positions.tolist() == [n0 % hb.period, n0 % hb.period, 0]
    # slot 1 goes on where it was, in one call with slot 0 again: equal to a run that never saw the skipped hops
    w2 = hb.width_out(1, n0 % hb.period)
    last0 = cut(long_rows[0], n0 + n1, n0 + n1 + 1, w0 + w1, w0 + w1 + w2)
    next1 = cut(long_rows[1], n0, n0 + 1, w0, w0 + w2)
    got = feed(hb, [last0, next1], (1,), slots=[0, 1])
    ref = _hb(2, rate, quality, lag_hops)
    want = feed(ref, [cut(r, 0, n0 + 1, 0, w0 + w2) for r in (long_rows[1], long_rows[1])], (n0 + 1,))
    assert np.array_equal(got[1], want[0][w0:])


@pytest.mark.parametrize('rate,quality,lag_hops', [(44100, 'high', 1), (44100, 'scipy', 1), (88200, 'high', 3)])
def test_reset_restarts_one_slot_and_leaves_the_others(rate, quality, lag_hops):
    rows, ys = run(rate, quality, lag_hops)
    hb = _hb(B, rate, quality, lag_hops)
    n0 = 3
    w0 = hb.width_out(n0, 0)
    head = [(r[0][:n0 * S.HOP], r[1][:n0 * S.HOP], r[2][:w0]) for r in rows[:2]]
    feed(hb, head, (n0,), slots=[0, 1])
    hb.reset([1], position=START2)
    fresh = _record(hb, 1)
    assert _lead(fresh) == HS.plan(rate, lag_hops, quality)['L0'] and not fresh[4:].any() and _record(hb, 0).any()
    assert hb.hops.tolist() == [n0, 0, 0] and hb.positions.tolist() == [n0, START2, 0]
    assert np.array_equal(feed(hb, rows[2:], GROUPS, slots=[1])[0], ys[2])   # as a fresh object started at that position
    tail = [(rows[0][0][n0 * S.HOP:], rows[0][1][n0 * S.HOP:], rows[0][2][w0:])]
    assert np.array_equal(feed(hb, tail, (HOPS - n0,), slots=[0])[0], ys[0][w0:])         # the neighbour never noticed


# ------------------------------------------------------------------------------------------------- 6. the guard
def test_a_lead_outside_its_bounds_gives_nan_and_keeps_the_record():
    """44.1 kHz: slot 1 given position 0 (a hop of 705 samples) call after call moves its lead by 705 x 160 - 256 x 441 = -96 per call.
    From L0 - s = -160 three such calls fit (-160, -256, -352 >= -E up = -441): their output is the conversion of what was fed from that
    lead, whatever the widths.  The fourth (L = -448) does not: NaN columns, the record byte-identical, the neighbours untouched."""
    hb = _hb(B, 44100, g=0.7)
    plan = HS.plan(44100, 1)
    assert (plan['L0'], plan['E'], hb.up, hb.down, hb.width_out(1, 0)) == (-160, 1, 441, 160, 705)
    enh, low, x = _signals(hb, (0,), 6, hops=5)[0]
    x = x[:4 * 705]
    neighbours = [_record(hb, 0), _record(hb, 2)]
    outs = []
    for call in range(4):
        hb.positions[:] = 0                                  # what the host's bookkeeping would never do
        before = _record(hb, 1)
        assert _lead(before) == -160 - 96 * call
        E, Lo, X = (torch.zeros((B, n), device='cuda') for n in (S.HOP, S.HOP, 705))
        E[1], Lo[1], X[1] = (torch.from_numpy(v).cuda() for v in (enh[call * 256:(call + 1) * 256], low[call * 256:(call + 1) * 256], x[call * 705:(call + 1) * 705]))
        out = torch.full((B, 705), SENTINEL, device='cuda')
        hb.process(E, Lo, X, active=[False, True, False], out=out)
        outs.append(out.cpu().numpy())
        assert (out[0] == SENTINEL).all() and (out[2] == SENTINEL).all()
        if call < 3:
            assert _lead(_record(hb, 1)) == -160 - 96 * (call + 1)
        else:
            assert np.isnan(outs[-1][1]).all() and torch.equal(_record(hb, 1), before)
    assert torch.equal(_record(hb, 0), neighbours[0]) and torch.equal(_record(hb, 2), neighbours[1])
    got = np.concatenate([o[1] for o in outs[:3]])
    g32 = np.float32(0.7)
    n16 = 3 * S.HOP
    d = fma32(-g32, _delayed(low[:n16], 256), enh[:n16]).astype(np.float64)
    u = HS.direct(d, 441, 160, _lib_taps(hb), -160, len(got))
    gx = _delayed(x[:len(got)], hb.lag)
    y64 = fma32(g32, gx, u.astype(np.float32)).astype(np.float64)
    bound = _bound(y64, d, g32 * gx) + np.spacing(np.abs(u).astype(np.float32)).astype(np.float64)
    worst = float((np.abs(got.astype(np.float64) - y64) / bound).max())
    print('three calls off the schedule: largest |gpu - reference| / bound = %.3f' % worst)
    assert np.isfinite(got).all() and worst <= 1.0


# ------------------------------------------------------------------------------------------------- 7. the wrapper by hand
def _generator():
    from nele_gan_amd import model
    G = model.Generator_Conv1D_cLN()
    sd = G.state_dict()
    arrs = seeded_state_arrays([(k, tuple(v.shape)) for k, v in sd.items()], 101)
    G.load_state_dict({k: torch.from_numpy(v) for k, v in arrs.items()})
    return G.cuda()


def _rt(G, streams):
    from nele_gan_amd.realtime import RealtimeEnhancer
    return RealtimeEnhancer(G=G, streams=streams, precision='f32', norm='prefix')


def _sr(streams, sr_in, sr_out):
    from nele_gan_amd.resample import ScheduledStreamResampler
    return ScheduledStreamResampler(streams, sr_in, sr_out)


def _device_signals(wrap, streams, hops, impulse_at, seed):
    """clean: a low Gaussian floor with one unit impulse per row; second: Gaussian noise; float32 at the device rate"""
    rs = np.random.RandomState(seed)
    n = wrap.width(hops, 0)
    clean = (1e-3 * rs.randn(streams, n)).astype(np.float32)
    for b, t in enumerate(impulse_at):
        clean[b, t] = 1.0
    return clean, (0.05 * rs.randn(streams, n)).astype(np.float32)


def _by_hand(rate, inner, clean, second, widths, lag_hops=1, g=1.0):
    """a ScheduledStreamResampler down on each signal and inner.process, call by call of ``widths``; then item 1's composition on the
    whole of enh, low and clean"""
    from nele_gan_amd.highband import highband_sched_plan
    Bw = clean.shape[0]
    dc, ds = _sr(Bw, rate, S.RATE), _sr(Bw, rate, S.RATE)
    lows, enhs, at = [], [], 0
    for w in widths:
        c16 = dc.process(torch.from_numpy(clean[:, at:at + w]))
        lows.append(c16.cpu())
        enhs.append(inner.process(c16, ds.process(torch.from_numpy(second[:, at:at + w]))).cpu())
        at += w
    assert at == clean.shape[1]
    plan = highband_sched_plan(rate, lag_hops)
    gt = torch.tensor(g, dtype=torch.float32)
    u = composed_u(rate, 'high', plan['shift'], torch.cat(enhs, dim=1) - gt * _delayed(torch.cat(lows, dim=1), plan['lag16']))
    return (u[:, :at] + gt * _delayed(torch.from_numpy(clean), plan['lag'])).numpy()


def test_adapt_fullband_at_44100_is_the_chain_by_hand():
    """B = 2, 7 hops in calls of (1, 2, 4) and drain"""
    from nele_gan_amd.highband import ScheduledHighBandUp
    from nele_gan_amd.streamrate import FullBandScheduledEnhancer, RateAdaptedEnhancer, adapt_fullband
    Bw, hops, rate = 2, 7, 44100
    G = _generator()
    wrap = adapt_fullband(_rt(G, Bw), rate)
    assert type(wrap) is FullBandScheduledEnhancer and type(wrap.up) is ScheduledHighBandUp and wrap.down.S == 2 * Bw and wrap.up.S == Bw
    assert wrap.latency == wrap.up.lag == 883 and wrap.up.shift == 32 and wrap.up.lag_hops == 1 and wrap.hop is None and wrap.highband == 1.0
    clean, second = _device_signals(wrap, Bw, hops, [805, 1443], 44)
    outs, at, h = [], 0, 0
    for g in (1, 2, 4):
        w = wrap.width(g)
        assert w == wrap.width(g, h % 5)
        outs.append(wrap.process(torch.from_numpy(clean[:, at:at + w]), torch.from_numpy(second[:, at:at + w])))
        assert outs[-1].shape == (Bw, w)                      # a call returns as many columns as it was given
        at, h = at + w, h + g
    assert at == clean.shape[1]
    outs.append(wrap.drain(range(Bw)))
    got = torch.cat(outs, dim=1).cpu().numpy()
    nd = 2                                                   # ceil(883 / 705.6)
    assert got.shape == (Bw, wrap.width(hops + nd, 0)) and wrap.down.position == wrap.up.position == hops % 5
    pad = np.zeros((Bw, wrap.width(nd, hops % 5)), np.float32)
    hand = _by_hand(rate, _rt(G, Bw), np.concatenate([clean, pad], axis=1), np.concatenate([second, pad], axis=1),
                    [wrap.width(1, k % 5) for k in range(hops + nd)])
    assert np.array_equal(_bits(got), _bits(hand))
    # reset: the wrapper starts again as a new one, at the position it is told
    wrap.reset(range(Bw), position=0)
    w = wrap.width(1, 0)
    again = wrap.process(torch.from_numpy(clean[:, :w]), torch.from_numpy(second[:, :w])).cpu().numpy()
    assert np.array_equal(_bits(again), _bits(got[:, :w]))
    # where RateAdaptedEnhancer serves the rate it is that class, and 16 kHz passes through
    a48, a16 = adapt_fullband(_rt(G, Bw), 48000, gain=0.5), adapt_fullband(_rt(G, Bw), 16000)
    assert type(a48) is RateAdaptedEnhancer and a48.highband == 0.5 and a48.latency == 960 and float(a48.up.gain[0]) == 0.5
    assert type(a16) is RateAdaptedEnhancer and a16.down is None and a16.up is None


def test_the_fullband_wrapper_around_the_echo_canceller():
    """44.1 kHz, P = 2, 2 hops per call: the wrapper around an EchoCancellingEnhancer against the converters and a second loop by hand"""
    from nele_gan_amd.aec import EchoCanceller, EchoCancellingEnhancer
    from nele_gan_amd.streamrate import adapt_fullband
    Bw, hops, rate = 2, 6, 44100
    G = _generator()
    wrap = adapt_fullband(EchoCancellingEnhancer(_rt(G, Bw), EchoCanceller(Bw, partitions=2)), rate, gain=0.5)
    assert wrap.latency == 883
    clean, mic = _device_signals(wrap, Bw, hops, [900, 1700], 45)
    got, at = [], 0
    for k in range(0, hops, 2):
        w = wrap.width(2)
        got.append(wrap.process(torch.from_numpy(clean[:, at:at + w]), torch.from_numpy(mic[:, at:at + w])))
        at += w
    got.append(wrap.drain([0, 1]))
    got = torch.cat(got, dim=1).cpu().numpy()
    pad = np.zeros((Bw, wrap.width(2, hops % 5)), np.float32)
    loop = EchoCancellingEnhancer(_rt(G, Bw), EchoCanceller(Bw, partitions=2))
    hand = _by_hand(rate, loop, np.concatenate([clean, pad], axis=1), np.concatenate([mic, pad], axis=1),
                    [wrap.width(2, k % 5) for k in range(0, hops + 2, 2)], g=0.5)
    assert got.shape == hand.shape == (Bw, wrap.width(hops + 2, 0))
    assert np.array_equal(_bits(got), _bits(hand))
    assert np.isfinite(got).all() and np.abs(got).max() > 0.0


def test_without_the_band_the_scheduled_wrapper_is_what_it_was():
    """ScheduledRateEnhancer: the down-converter, the enhancer and the plain up-converter, bit for bit, and the latency of before"""
    from fractions import Fraction
    from nele_gan_amd.resample import ScheduledStreamResampler
    from nele_gan_amd.streamrate import ScheduledRateEnhancer, adapt
    Bw, hops, rate = 2, 4, 44100
    G = _generator()
    wrap, via = ScheduledRateEnhancer(_rt(G, Bw), rate), adapt(_rt(G, Bw), rate)
    assert type(via) is ScheduledRateEnhancer and type(wrap.up) is ScheduledStreamResampler and wrap.highband is None
    assert wrap.latency == via.latency == Fraction(4414, 5)
    clean, second = _device_signals(wrap, Bw, hops, [800, 1700], 46)
    dc, dn, rt, up = _sr(Bw, rate, S.RATE), _sr(Bw, rate, S.RATE), _rt(G, Bw), _sr(Bw, S.RATE, rate)
    c, s = torch.from_numpy(clean), torch.from_numpy(second)
    hand = up.process(rt.process(dc.process(c), dn.process(s))).cpu().numpy()
    for w in (wrap, via):
        assert np.array_equal(_bits(w.process(c, s).cpu().numpy()), _bits(hand))


# ------------------------------------------------------------------------------------------------- 8. the point of it
def test_an_18_khz_tone_passes_the_wrapper_at_44100_only_with_the_band():
    """B = 2, 40 hops at 44.1 kHz: clean = a unit 18 kHz sinusoid + 0.5 of a 1 kHz one, noise a 1e-3 Gaussian floor.  The output is
    projected onto the 18 kHz sinusoid delayed by ``latency`` over hops 10 .. 39: 21168 samples, 8640 and 480 periods."""
    from nele_gan_amd.streamrate import FullBandScheduledEnhancer, ScheduledRateEnhancer
    Bw, hops, rate, f = 2, 40, 44100, 18000.0
    G = _generator()
    n, n0 = 40 * 3528 // 5, 10 * 3528 // 5
    m = np.arange(n)
    clean = (np.sin(2.0 * np.pi * f * m / rate) + 0.5 * np.sin(2.0 * np.pi * 1000.0 * m / rate)).astype(np.float32)[None].repeat(Bw, axis=0)
    noise = (1e-3 * np.random.RandomState(18).randn(Bw, n)).astype(np.float32)
    win = slice(n0, n)
    assert ((n - n0) * f / rate) % 1.0 == 0.0 and ((n - n0) * 1000.0 / rate) % 1.0 == 0.0
    amps = {}
    for gain in (1.0, None, 0.5):
        wrap = ScheduledRateEnhancer(_rt(G, Bw), rate) if gain is None else FullBandScheduledEnhancer(_rt(G, Bw), rate, gain=gain)
        assert wrap.width(hops, 0) == n and (gain is None or wrap.latency == 883)
        lat = 883                                            # the plain wrapper's 882.8 samples: what it leaves is measured as a magnitude
        outs, at = [], 0
        for k in range(0, hops, 8):
            w = wrap.width(8)
            outs.append(wrap.process(torch.from_numpy(clean[:, at:at + w]), torch.from_numpy(noise[:, at:at + w])))
            at += w
        out = torch.cat(outs, dim=1).cpu().numpy().astype(np.float64)
        ref_s, ref_c = np.sin(2.0 * np.pi * f * (m - lat) / rate)[win], np.cos(2.0 * np.pi * f * (m - lat) / rate)[win]
        amps[gain] = [(2.0 * np.mean(out[b, win] * ref_s), 2.0 * np.mean(out[b, win] * ref_c)) for b in range(Bw)]
        print('gain=%s: 18 kHz in phase / quadrature per row: %s' % (gain, ['%.9f / %.3g' % ab for ab in amps[gain]]))
    for b in range(Bw):
        assert abs(amps[1.0][b][0] - 1.0) <= 1e-5 and abs(amps[1.0][b][1]) <= 1e-5
        assert np.hypot(*amps[None][b]) < 1e-5
        assert abs(amps[0.5][b][0] - 0.5) <= 1e-5 and abs(amps[0.5][b][1]) <= 1e-5


@pytest.mark.parametrize('lag_hops', [1, 2])
def test_an_impulse_comes_out_latency_samples_later(lag_hops):
    """44.1 kHz: a unit impulse in ``clean`` over the floor comes out exactly ``latency`` samples later; lag_hops 2 is an
    EchoCancellingEnhancer around a CompressedEnhancer."""
    from nele_gan_amd.aec import EchoCanceller, EchoCancellingEnhancer
    from nele_gan_amd.drc import CompressedEnhancer, StreamCompressor
    from nele_gan_amd.streamrate import adapt_fullband
    Bw, hops, rate = 2, 6, 44100
    G = _generator()
    inner = _rt(G, Bw) if lag_hops == 1 else EchoCancellingEnhancer(CompressedEnhancer(_rt(G, Bw), StreamCompressor(Bw)), EchoCanceller(Bw, partitions=2))
    wrap = adapt_fullband(inner, rate)
    assert wrap.up.lag_hops == lag_hops and wrap.latency == {1: 883, 2: 1589}[lag_hops]
    t0 = [705 + 300, 1411 + 99]
    clean, second = _device_signals(wrap, Bw, hops, t0, 47)
    outs, at = [], 0
    for k in range(0, hops, 2):
        w = wrap.width(2)
        outs.append(wrap.process(torch.from_numpy(clean[:, at:at + w]), torch.from_numpy(second[:, at:at + w])))
        at += w
    got = torch.cat(outs, dim=1).cpu().numpy()
    peaks = [int(np.abs(got[b]).argmax()) - t0[b] for b in range(Bw)]
    print('lag_hops %d: impulses at %s, peaks of |out| %s samples later, latency %d' % (lag_hops, t0, peaks, wrap.latency))
    assert peaks == [wrap.latency] * Bw
