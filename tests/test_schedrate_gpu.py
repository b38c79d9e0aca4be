"""GPU: the scheduled stream converter (nele_gan_amd/resample.py ScheduledStreamResampler, csrc/resample_sched.hip) and
ScheduledRateEnhancer (nele_gan_amd/streamrate.py) against DESIGN.md section 20: bit identity with the offline kernel (Resampler.apply of
the whole signal, delayed by D) from two starting positions of the schedule, tests/schedrate_ref.py in float64, the streaming contract
(grouping, batch, slots, reset: bitwise), section 15's converter at the whole-hop rates (bitwise), the guard, a closed form, and the
wrapper against the chain built by hand (bitwise).

Bounds.  Against the offline kernel and StreamResampler: equal bits.  Against float64: resample_ref.bound per sample - one float32 ulp of
the float64 result plus 1e-12 max |x| (the bound of the two existing GPU resampler tests).  Sinusoid: 1e-5 (section 12's bound: float32
samples of a unit sinusoid through a filter whose pass-band ripple at 1 kHz is below 1e-6).  Impulse through the wrapper: the peak of
|out| within one sample of the (fractional) latency.
Measured on an MI355X: bit-equal to the offline kernel in all 12 cases (6 pairs, both presets) from both starting positions, flush
included; largest |gpu - float64| / bound 0.500 in every case - half a float32 ulp, the rounding of the stored sample itself; 1 kHz
sinusoid 4.75e-8 (44.1 -> 16 kHz; offline 4.8e-8) and 7.83e-6 (16 -> 44.1 kHz); impulse peaks 883 samples late at 44.1 kHz (805 -> 1688,
1443 -> 2326; latency 882.8) and 441 at 22.05 kHz (452 -> 893, 737 -> 1178; latency 440.9); the whole file runs in 3 s."""
import ctypes

import numpy as np
import pytest

import resample_ref as R
import schedrate_ref as S

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from test_streamrate_gpu import _generator, _rt  # noqa: E402  (the seeded generator and its RealtimeEnhancer)

B, HOPS, GROUPS, SENTINEL, START2 = 3, 7, (3, 4), -7.25, 2
FAMILY = [p for p in S.FAMILY if 88200 not in p]
CASES = [(a, b, q) for a, b in FAMILY for q in sorted(S.PRESETS)]
THREE = [(44100, 16000), (16000, 44100), (11025, 16000)]
_RUNS = {}


def _sr(streams, sr_in, sr_out, quality='high', position=0):
    from nele_gan_amd.resample import ScheduledStreamResampler
    sr = ScheduledStreamResampler(streams, sr_in, sr_out, quality)
    if position:
        sr.reset(range(streams), position=position)
    return sr


def _signals(sr, starts, seed, hops=HOPS):
    """float32 Gaussian rows of ``hops`` hops from the schedule positions ``starts``, row 1 scaled by 1e-6 and row 2 by 1e3"""
    rs = np.random.RandomState(seed)
    xs = [rs.randn(sr.width_in(hops, g)).astype(np.float32) for g in starts]
    for row, scale in ((1, 1e-6), (2, 1e3)):
        if row < len(xs):
            xs[row] *= np.float32(scale)
    return xs


def feed(sr, xs, groups, slots=None, out=False):
    """the rows xs (one per slot of ``slots``, default all; those slots stand at one position) through ``sr``, ``groups`` hops per call
    in turn -> [len(slots), ..] on the host"""
    slots = list(range(sr.S)) if slots is None else slots
    active = None if len(slots) == sr.S else [s in slots for s in range(sr.S)]
    ys, at = [], 0
    for g in groups:
        pos = int(sr.positions[slots[0]])
        w = sr.width_in(g, pos)
        X = np.zeros((sr.S, w), dtype=np.float32)
        for k, s in enumerate(slots):
            X[s] = xs[k][at:at + w]
        buf = torch.full((sr.S, sr.width_out(g, pos)), SENTINEL, device='cuda') if out else None
        y = sr.process(torch.from_numpy(X), active=active, out=buf)
        assert buf is None or y is buf
        assert y.shape == (sr.S, sr.width_out(g, pos))
        ys.append(y.cpu().numpy()[slots])
        at += w
    assert all(at == len(x) for x in xs)
    return np.concatenate(ys, axis=1)


def run(sr_in, sr_out, quality):
    """(xs [B rows], emitted [B rows], flushed [B rows of D]) of the case: slots 0 and 1 from position 0 and slot 2, reset to position
    START2, from there in calls of its own, each HOPS hops in calls of GROUPS: one GPU run, shared, never changed"""
    key = (sr_in, sr_out, quality)
    if key not in _RUNS:
        sr = _sr(B, sr_in, sr_out, quality)
        assert sr.period == 5 and sr.position == 0
        sr.reset([2], position=START2)
        assert sr.positions.tolist() == [0, 0, START2]
        xs = _signals(sr, (0, 0, START2), sr_in // 100 + sr_out // 1000 + len(quality))
        y01 = feed(sr, xs[:2], GROUPS, slots=[0, 1])
        assert sr.position == HOPS % 5 and sr.positions.tolist() == [HOPS % 5, HOPS % 5, START2]
        y2 = feed(sr, xs[2:], GROUPS, slots=[2])
        assert sr.hops.tolist() == [HOPS] * B and sr.positions[2] == (START2 + HOPS) % 5
        t01 = sr.flush([0, 1]).cpu().numpy()
        t2 = sr.flush([2]).cpu().numpy()
        assert (sr.hops == 0).all()
        _RUNS[key] = (xs, [y01[0], y01[1], y2[0]], [t01[0], t01[1], t2[0]], sr)
    return _RUNS[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _offline(sr_in, sr_out, quality, x, pad):
    """Resampler.apply of x and ``pad`` zeros behind it (what flush feeds), on the host"""
    from nele_gan_amd.resample import Resampler
    z = np.concatenate([x, np.zeros(pad, dtype=np.float32)])
    whole, n = Resampler(sr_in, sr_out, quality).apply(torch.from_numpy(z[None]).cuda(), [len(z)])
    return whole[0, :int(n[0])].cpu().numpy()


# ------------------------------------------------------------------------------------------------- 1. the offline kernel, delayed by D
@pytest.mark.parametrize('sr_in,sr_out,quality', CASES)
def test_bit_identical_to_the_offline_resampler(sr_in, sr_out, quality):
    xs, ys, tails, sr = run(sr_in, sr_out, quality)
    D = sr.delay
    for b in range(B):
        T = len(ys[b])
        assert T == (HOPS * 256 if sr.to16k else len(ys[b])) and tails[b].shape == (D,)
        whole = _offline(sr_in, sr_out, quality, xs[b], sr.width_in(1, 0) + 1)
        assert len(whole) >= T
        assert np.array_equal(_bits(ys[b][D:]), _bits(whole[:T - D])), b
        assert np.array_equal(_bits(tails[b]), _bits(whole[T - D:T])), b
        assert np.abs(ys[b][:D]).max() > 0.0


# ------------------------------------------------------------------------------------------------- 2. float64
@pytest.mark.parametrize('sr_in,sr_out,quality', CASES)
def test_against_the_float64_reference(sr_in, sr_out, quality):
    from nele_gan_amd.resample import taps
    xs, ys, tails, sr = run(sr_in, sr_out, quality)
    h = taps(sr.up, sr.down, sr.zeros, sr.beta)
    worst = 0.0
    for b, start in enumerate((0, 0, START2)):
        ref = S.SchedRef(sr.up, sr.down, h, sr.to16k, start)
        assert (ref.D, ref.K, ref.H, ref.P) == (sr.delay, sr.K, sr.H, sr.period)
        y64 = np.concatenate([ref.run(xs[b]), ref.flush()])
        got = np.concatenate([ys[b], tails[b]]).astype(np.float64)
        assert got.shape == y64.shape
        worst = max(worst, float((np.abs(got - y64) / R.bound(y64, float(np.abs(xs[b]).max()))).max()))
    print('%d -> %d %s: largest |gpu - float64| / bound = %.3f' % (sr_in, sr_out, quality, worst))
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------- 3. grouping and batch
@pytest.mark.parametrize('sr_in,sr_out', THREE)
def test_hop_grouping_batch_and_out_buffer_do_not_change_a_slot(sr_in, sr_out):
    xs, ys, _, _ = run(sr_in, sr_out, 'high')                 # calls of (3, 4) hops
    for groups, out in (((1,) * HOPS, False), ((4, 3), True), ((HOPS,), False)):
        got = feed(_sr(2, sr_in, sr_out), xs[:2], groups, out=out)
        assert np.array_equal(_bits(got[0]), _bits(ys[0])) and np.array_equal(_bits(got[1]), _bits(ys[1])), groups
        got = feed(_sr(1, sr_in, sr_out, position=START2), xs[2:], groups, out=out)          # a stream alone, from another position
        assert np.array_equal(_bits(got[0]), _bits(ys[2])), groups
    five = _sr(5, sr_in, sr_out, position=START2)
    others = _signals(five, (START2,) * 5, 99)[::-1]
    others[3] = xs[2]
    assert np.array_equal(_bits(feed(five, others, (1, 2, 4))[3]), _bits(ys[2]))


# ------------------------------------------------------------------------------------------------- 4. the whole-hop rates
@pytest.mark.parametrize('sr_in,sr_out', S.WHOLE)
@pytest.mark.parametrize('quality', sorted(S.PRESETS))
def test_whole_hop_rates_are_section_15s_converter(sr_in, sr_out, quality):
    from nele_gan_amd.resample import StreamResampler
    new, old = _sr(B, sr_in, sr_out, quality), StreamResampler(B, sr_in, sr_out, quality)
    assert (new.period, new.delay, new.K, new.H) == (1, old.delay, old.K, old.K - 1)
    assert (new.width_in(1), new.width_out(1)) == (old.hop_in, old.hop_out)
    xs = _signals(new, (0,) * B, sr_in // 1000, hops=5)
    got = feed(new, xs, (2, 3))
    want = torch.cat([old.process(torch.from_numpy(np.stack(xs)[:, :2 * old.hop_in])), old.process(torch.from_numpy(np.stack(xs)[:, 2 * old.hop_in:]))],
                     dim=1).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(new.flush(range(B)).cpu().numpy()), _bits(old.flush(range(B)).cpu().numpy()))


# ------------------------------------------------------------------------------------------------- 5. slots
def _record(sr, slot):
    from nele_gan_amd import _lib
    rec = int(_lib.lib.nele_sched_stream_record_bytes(sr.H))
    assert sr.nbytes - sr.S * rec == 256
    return sr.state[256 + slot * rec:256 + (slot + 1) * rec].clone()


def _lead(record):
    return int(record[:4].cpu().numpy().view(np.int32)[0])


@pytest.mark.parametrize('sr_in,sr_out', THREE[:2])
def test_inactive_slots_are_neither_read_nor_written(sr_in, sr_out):
    """slot 1 sits out one period of the schedule (5 hops) and is in step again"""
    sr = _sr(B, sr_in, sr_out)
    n0, n1, n2 = 2, sr.period, 2
    xs = _signals(sr, (0, 0, 0), 5, hops=n0 + n1 + n2)
    want = [feed(_sr(1, sr_in, sr_out), [x], (n0 + n1 + n2,))[0] for x in (xs[0], xs[2])]
    w0, w1 = sr.width_in(n0, 0), sr.width_in(n1, n0)
    x1 = np.concatenate([xs[1][:w0], xs[1][w0 + w1:]])         # slot 1 never sees the middle
    want1 = feed(_sr(1, sr_in, sr_out), [x1[:w0]], (n0,))[0]
    first = feed(sr, [xs[0][:w0], xs[1][:w0], xs[2][:w0]], (n0,))
    assert np.array_equal(_bits(first[1]), _bits(want1))
    before = _record(sr, 1)
    assert before[16:].any()
    X = np.stack([xs[0][w0:w0 + w1], np.full(w1, np.nan, np.float32), xs[2][w0:w0 + w1]])
    out = torch.full((B, sr.width_out(n1, n0)), SENTINEL, device='cuda')
    sr.process(torch.from_numpy(X), active=[True, False, True], out=out)
    assert (out[1] == SENTINEL).all() and not (out[0] == SENTINEL).any() and not (out[2] == SENTINEL).any()
    assert torch.equal(_record(sr, 1), before)
    assert sr.positions.tolist() == [(n0 + n1) % 5, n0, (n0 + n1) % 5] and sr.hops.tolist() == [n0 + n1, n0, n0 + n1]
    # slot 1 goes on where it was, in one call with the others: equal to a run that never saw the skipped call
    rest = feed(sr, [xs[0][w0 + w1:], x1[w0:], xs[2][w0 + w1:]], (n2,))
    lone = _sr(1, sr_in, sr_out)
    ref1 = feed(lone, [x1], (n0, n2))[0]
    assert np.array_equal(_bits(rest[1]), _bits(ref1[len(want1):]))
    o0 = sr.width_out(n0, 0) + sr.width_out(n1, n0)
    assert np.array_equal(_bits(out.cpu().numpy()[[0, 2]]), _bits(np.stack(want)[:, sr.width_out(n0, 0):o0]))
    assert np.array_equal(_bits(rest[[0, 2]]), _bits(np.stack(want)[:, o0:]))


@pytest.mark.parametrize('sr_in,sr_out', THREE[:2])
def test_reset_restarts_one_slot_at_the_running_position_and_leaves_the_others(sr_in, sr_out):
    sr = _sr(B, sr_in, sr_out)
    n0, n1 = 2, 3
    xs = _signals(sr, (0, 0, 0), 6, hops=n0 + n1)
    whole = feed(_sr(B, sr_in, sr_out), xs, (n0 + n1,))
    w0 = sr.width_in(n0, 0)
    feed(sr, [x[:w0] for x in xs], (n0,))
    keep = [_record(sr, 0), _record(sr, 2)]
    sr.reset([1])
    rec = _record(sr, 1)
    assert _lead(rec) == S.plan(sr.up, sr.down, sr.zeros, sr.to16k)['L0'] and not rec[4:].any()
    assert torch.equal(_record(sr, 0), keep[0]) and torch.equal(_record(sr, 2), keep[1])
    assert sr.hops.tolist() == [n0, 0, n0] and sr.positions.tolist() == [n0] * 3 and sr.position == n0
    fresh = _signals(sr, (n0,), 7, hops=n1)[0]
    got = feed(sr, [xs[0][w0:], fresh, xs[2][w0:]], (1, 2))
    assert np.array_equal(_bits(got[1]), _bits(feed(_sr(1, sr_in, sr_out, position=n0), [fresh], (n1,))[0]))      # as a fresh converter there
    assert np.array_equal(_bits(got[[0, 2]]), _bits(whole[[0, 2], sr.width_out(n0, 0):]))                         # the neighbours never noticed


# ------------------------------------------------------------------------------------------------- 6. the guard
def test_a_lead_outside_its_bounds_gives_nan_and_keeps_the_record():
    """44.1 -> 16 kHz through the C entry point.  Slot 1 is given position 1 (hops of 706 samples) call after call: each such hop moves
    its lead by 256 * 441 - 706 * 160 = -64, and the stream stays the offline conversion of what it was fed while the lead is inside
    its bounds (-E up = -160 <= L, L + 255 * 441 < 706 * 160).  The reference says how many such calls fit - three, leads 0, -64, -128 -
    and that the fourth (L = -192) does not: there the kernel reads the lead alone, stores NaN in the slot's columns and returns."""
    from nele_gan_amd import _lib
    from nele_gan_amd.resample import taps
    sr_in, sr_out = 44100, 16000
    sr = _sr(B, sr_in, sr_out)
    ref = S.SchedRef(sr.up, sr.down, taps(sr.up, sr.down, sr.zeros, sr.beta), True)
    n_in, n_out = S.widths(sr.up, sr.down, True, 1, 1)
    assert (n_in, n_out) == (706, 256)
    L, fits = ref.L0, 0
    while ref.in_bounds(n_in, n_out, L) and fits < 100:
        L, fits = L + n_out * sr.down - n_in * sr.up, fits + 1
    assert (fits, L) == (3, -192) and L < -ref.E * sr.up

    def hop(x, active, y):
        xd, ad = torch.from_numpy(np.ascontiguousarray(x)).cuda(), torch.from_numpy(np.asarray(active, dtype=np.uint8)).cuda()
        _lib.call('nele_sched_stream_hop', _lib.ptr(sr.state), ctypes.c_longlong(sr.nbytes), B, sr.up, sr.down, sr.K, 1, _lib.ptr(sr.table),
                  _lib.ptr(xd), ctypes.c_longlong(n_in), _lib.ptr(ad), 1, 1, _lib.ptr(y), ctypes.c_longlong(n_out), _lib.stream())
        torch.cuda.synchronize()
        return y.cpu().numpy()

    x = np.random.RandomState(11).randn(B, (fits + 1) * n_in).astype(np.float32)
    got = []
    for k in range(fits):                                     # inside the bounds: as the schedule of these widths says
        y = hop(x[:, k * n_in:(k + 1) * n_in], [0, 1, 0], torch.full((B, n_out), SENTINEL, device='cuda'))
        assert (y[[0, 2]] == SENTINEL).all() and np.isfinite(y[1]).all()
        got.append(y[1])
    got = np.concatenate(got)
    whole = _offline(sr_in, sr_out, 'high', x[1, :fits * n_in], n_in)
    assert np.array_equal(_bits(got[sr.delay:]), _bits(whole[:len(got) - sr.delay]))
    before = [_record(sr, b) for b in range(B)]
    assert _lead(before[1]) == L and _lead(before[0]) == _lead(before[2]) == ref.L0
    y = hop(x[:, fits * n_in:], [1, 1, 1], torch.full((B, n_out), SENTINEL, device='cuda'))
    assert np.isnan(y[1]).all() and np.isfinite(y[[0, 2]]).all() and not (y[[0, 2]] == SENTINEL).any()
    assert torch.equal(_record(sr, 1), before[1])
    assert _lead(_record(sr, 0)) == _lead(_record(sr, 2)) == ref.L0 + n_out * sr.down - n_in * sr.up
    lone = _sr(2, sr_in, sr_out, position=1)                  # the neighbours: as a converter that stands at position 1
    want = lone.process(torch.from_numpy(x[[0, 2], fits * n_in:])).cpu().numpy()
    assert np.array_equal(_bits(y[[0, 2]]), _bits(want))


# ------------------------------------------------------------------------------------------------- 7. a closed form
@pytest.mark.parametrize('sr_in,sr_out', THREE[:2])
def test_a_sinusoid_comes_out_as_that_sinusoid_shifted_by_D(sr_in, sr_out):
    hops, f = 32, 1000.0
    sr = _sr(1, sr_in, sr_out)
    x = np.sin(2.0 * np.pi * f * np.arange(sr.width_in(hops, 0)) / sr_in).astype(np.float32)
    y = feed(sr, [x], (7, 25))[0].astype(np.float64)
    assert len(y) == sr.width_out(hops, 0)
    want = np.sin(2.0 * np.pi * f * (np.arange(len(y)) - sr.delay) / sr_out)
    skip = 72 + sr.delay
    err = float(np.abs(y - want)[skip:].max())
    print('%d -> %d: 1 kHz sinusoid, largest error behind output %d: %.3g' % (sr_in, sr_out, skip, err))
    assert err <= 1e-5


# ------------------------------------------------------------------------------------------------- 8. ScheduledRateEnhancer
def _device_signals(wrap, streams, hops, impulse_at, seed):
    """clean: a low Gaussian floor with one unit impulse per row; second: Gaussian noise; float32 at the device rate"""
    rs = np.random.RandomState(seed)
    n = wrap.width(hops, 0)
    clean = (1e-3 * rs.randn(streams, n)).astype(np.float32)
    for b, t in enumerate(impulse_at):
        clean[b, t] = 1.0
    return clean, (0.05 * rs.randn(streams, n)).astype(np.float32)


def _by_hand(rate, inner, clean, second, widths):
    """a ScheduledStreamResampler down on each signal, inner.process, a ScheduledStreamResampler up, call by call of ``widths``"""
    Bw = clean.shape[0]
    dc, ds, up = _sr(Bw, rate, S.RATE), _sr(Bw, rate, S.RATE), _sr(Bw, S.RATE, rate)
    outs, at = [], 0
    for w in widths:
        c16 = dc.process(torch.from_numpy(clean[:, at:at + w]))
        s16 = ds.process(torch.from_numpy(second[:, at:at + w]))
        outs.append(up.process(inner.process(c16, s16)))
        assert outs[-1].shape == (Bw, w)
        at += w
    return torch.cat(outs, dim=1).cpu().numpy(), dc, up


@pytest.mark.parametrize('rate', [44100, 22050])
def test_scheduled_rate_enhancer_is_the_chain_by_hand(rate):
    """B = 2, 7 hops in calls of (1, 2, 4) and drain; by hand hop by hop.  The impulse of each row comes out ``latency`` samples later,
    to within a sample: the latency is a fraction (882.8 samples at 44.1 kHz)."""
    from fractions import Fraction
    from nele_gan_amd.streamrate import ScheduledRateEnhancer
    Bw, hops = 2, 7
    G = _generator()
    wrap = ScheduledRateEnhancer(_rt(G, Bw), rate)
    assert wrap.down.S == 2 * Bw and wrap.up.S == Bw and wrap.down.period == wrap.up.period == 5
    r = Fraction(256 * rate, S.RATE)
    hop = int(r)
    t0 = [hop + 100, 2 * hop + 33]
    clean, second = _device_signals(wrap, Bw, hops, t0, rate // 1000)
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
    nd = -(-wrap.latency // r)
    assert wrap.latency == wrap.down.delay * r / 256 + r + wrap.up.delay and isinstance(wrap.latency, Fraction)
    if rate == 44100:
        assert wrap.latency == Fraction(4414, 5) and nd == 2
    assert got.shape == (Bw, wrap.width(hops + nd, 0))
    assert wrap.down.position == wrap.up.position == hops % 5                    # drain leaves ``position`` where process() put it
    # ---- by hand, hop by hop
    pad = np.zeros((Bw, wrap.width(nd, hops % 5)), np.float32)
    hand, dc, up = _by_hand(rate, _rt(G, Bw), np.concatenate([clean, pad], axis=1), np.concatenate([second, pad], axis=1),
                            [wrap.width(1, g % 5) for g in range(hops + nd)])
    assert np.array_equal(_bits(got), _bits(hand))
    assert (dc.delay, up.delay) == (wrap.down.delay, wrap.up.delay)
    for b in range(Bw):
        peak = int(np.abs(got[b]).argmax())
        print('%d Hz row %d: impulse at %d, peak of |out| at %d, latency %s = %.1f' % (rate, b, t0[b], peak, wrap.latency, float(wrap.latency)))
        assert abs(peak - t0[b] - wrap.latency) <= 1
    # ---- reset: the wrapper starts again as a new one, at the position it is told
    wrap.reset(range(Bw), position=0)
    w = wrap.width(1, 0)
    again = wrap.process(torch.from_numpy(clean[:, :w]), torch.from_numpy(second[:, :w])).cpu().numpy()
    assert np.array_equal(_bits(again), _bits(got[:, :w]))


def test_scheduled_rate_enhancer_around_the_echo_canceller():
    """44.1 kHz, 2 partitions, 2 hops per call: the wrapper around an EchoCancellingEnhancer against the converters and a second loop by hand"""
    from nele_gan_amd.aec import EchoCanceller, EchoCancellingEnhancer
    from nele_gan_amd.streamrate import ScheduledRateEnhancer
    Bw, hops, rate = 2, 6, 44100
    G = _generator()
    wrap = ScheduledRateEnhancer(EchoCancellingEnhancer(_rt(G, Bw), EchoCanceller(Bw, partitions=2)), rate)
    clean, mic = _device_signals(wrap, Bw, hops, [900, 1700], 44)
    got, at = [], 0
    for k in range(0, hops, 2):
        w = wrap.width(2)
        got.append(wrap.process(torch.from_numpy(clean[:, at:at + w]), torch.from_numpy(mic[:, at:at + w])))
        at += w
    got.append(wrap.drain([0, 1]))
    got = torch.cat(got, dim=1).cpu().numpy()
    pad = np.zeros((Bw, wrap.width(2, hops % 5)), np.float32)
    loop = EchoCancellingEnhancer(_rt(G, Bw), EchoCanceller(Bw, partitions=2))
    hand, _, _ = _by_hand(rate, loop, np.concatenate([clean, pad], axis=1), np.concatenate([mic, pad], axis=1),
                          [wrap.width(2, g % 5) for g in range(0, hops + 2, 2)])
    assert got.shape == hand.shape == (Bw, wrap.width(hops + 2, 0))
    assert np.array_equal(_bits(got), _bits(hand))
    assert np.isfinite(got).all() and np.abs(got).max() > 0.0


def test_adapt_picks_the_wrapper_that_serves_the_rate():
    from nele_gan_amd.streamrate import RateAdaptedEnhancer, ScheduledRateEnhancer, adapt
    rt = _rt(_generator(), 2)
    a48, a44, a16 = adapt(rt, 48000), adapt(rt, 44100), adapt(rt, 16000)
    assert type(a48) is RateAdaptedEnhancer and a48.hop == 768
    assert type(a44) is ScheduledRateEnhancer and a44.width(5) == 3528
    assert type(a16) is RateAdaptedEnhancer and a16.down is None and a16.up is None
    x = np.random.RandomState(3).randn(2, 512).astype(np.float32)
    direct = _rt(_generator(), 2).process(torch.from_numpy(x), torch.from_numpy(x[::-1].copy())).cpu().numpy()
    assert np.array_equal(_bits(a16.process(torch.from_numpy(x), torch.from_numpy(x[::-1].copy())).cpu().numpy()), _bits(direct))


# ------------------------------------------------------------------------------------------------- 9. errors
def test_errors_are_value_errors_before_any_launch():
    from nele_gan_amd.streamrate import ScheduledRateEnhancer
    sr = _sr(B, 44100, 16000)
    sr.reset([2], position=3)
    feed(sr, _signals(sr, (0, 0), 1, hops=1), (1,), slots=[0, 1])
    before, positions, hops = sr.state.clone(), sr.positions.copy(), sr.hops.copy()
    assert positions.tolist() == [1, 1, 3] and sr.position == 1
    good = torch.zeros((B, 706))
    two = [True, True, False]
    with pytest.raises(ValueError, match='width'):
        sr.process(torch.zeros((B, 705)), active=two)         # position 1 has 706
    with pytest.raises(ValueError, match='x must be'):
        sr.process(torch.zeros((B + 1, 706)), active=two)
    with pytest.raises(ValueError, match='x must be float32'):
        sr.process(good.double(), active=two)
    with pytest.raises(ValueError, match='active'):
        sr.process(good, active=[True] * (B + 1))
    with pytest.raises(ValueError, match='out must be'):
        sr.process(good, active=two, out=torch.zeros((B, 255), device='cuda'))
    with pytest.raises(ValueError, match='out must be'):
        sr.process(good, active=two, out=torch.zeros((B, 256), dtype=torch.float64, device='cuda'))
    with pytest.raises(ValueError, match=r'slots \[2\] stand at schedule positions \[3\]'):
        sr.process(good)
    with pytest.raises(ValueError, match=r'slots \[2\]'):
        sr.flush([0, 2])
    with pytest.raises(ValueError, match='position'):
        sr.reset([0], position=5)
    assert torch.equal(sr.state, before) and (sr.positions == positions).all() and (sr.hops == hops).all() and sr.position == 1
    rt = _rt(_generator(), 2)
    with pytest.raises(ValueError, match='inner'):
        ScheduledRateEnhancer(sr, 44100)
    wrap = ScheduledRateEnhancer(rt, 44100)
    ok = torch.zeros((2, 705))
    with pytest.raises(ValueError, match='width'):
        wrap.process(torch.zeros((2, 706)), torch.zeros((2, 706)))
    with pytest.raises(ValueError, match='second must be'):
        wrap.process(ok, torch.zeros((2, 1411)))
    with pytest.raises(ValueError, match='second must be float32'):
        wrap.process(ok, ok.double())
    with pytest.raises(ValueError, match='active'):
        wrap.process(ok, ok, active=[True])
    wrap.down.positions[:] = [0, 1, 0, 1]
    wrap.up.positions[:] = [0, 1]
    with pytest.raises(ValueError, match='slots'):
        wrap.process(ok, ok)
    assert not wrap.down.hops.any() and not wrap.up.hops.any() and not rt.hops.any()
    assert wrap.down.position == wrap.up.position == 0
