"""GPU: the stream converter (nele_gan_amd/resample.py StreamResampler, csrc/resample_stream.hip) and RateAdaptedEnhancer
(nele_gan_amd/streamrate.py) against DESIGN.md section 15: bit identity with the offline kernel (Resampler.apply of the whole signal,
delayed by D), tests/streamrate_ref.py in float64, the streaming contract (grouping, batch, slots, reset: bitwise), a closed form, and
the wrapper against the chain built by hand (bitwise).

Bounds.  Against the offline kernel: equal bits.  Against float64: resample_ref.bound per sample - one float32 ulp of the float64 result
plus 1e-12 max |x| (the offline GPU test's bound).  Sinusoid: 1e-5 (section 12's bound: float32 samples of a unit sinusoid through a
filter whose pass-band ripple at 1 kHz is below 1e-6).
Measured on an MI355X: bit-equal to the offline kernel in all 22 cases (11 pairs, both presets), flush included; largest
|gpu - float64| / bound 0.500 in every case, the first D and the flushed D outputs included - half a float32 ulp, the rounding of the
stored sample itself; 1 kHz sinusoid 2.83e-8 (48 -> 16 kHz) and 2.38e-7 (8 -> 16 kHz); impulse peaks exactly ``latency`` samples late
(1068 -> 2028, 1635 -> 2595 at 48 kHz; 228 -> 420, 289 -> 481 at 8 kHz); the whole file runs in 3 s."""
import numpy as np
import pytest

import resample_ref as R
import streamrate_ref as S

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from weights_recipe import seeded_state_arrays  # noqa: E402

B, HOPS, SENTINEL = 3, 5, -7.25
CASES = [(a, b, q) for a, b in S.PAIRS for q in sorted(S.PRESETS)]
_RUNS = {}


def _sr(streams, sr_in, sr_out, quality='high'):
    from nele_gan_amd.resample import StreamResampler
    return StreamResampler(streams, sr_in, sr_out, quality)


def _signal(sr_in, sr_out, quality, rows=B, hops=HOPS):
    """float32 Gaussian rows of ``hops`` hops, row 1 scaled by 1e-6 and row 2 by 1e3"""
    from nele_gan_amd.resample import stream_plan
    n_in = stream_plan(sr_in, sr_out, quality)['hop_in']
    x = np.random.RandomState(sr_in // 100 + sr_out // 1000 + len(quality)).randn(rows, hops * n_in).astype(np.float32)
    if rows > 1:
        x[1] *= np.float32(1e-6)
    if rows > 2:
        x[2] *= np.float32(1e3)
    return x


def feed(sr, x, groups, slots=None, out=False):
    """the columns of x [n, hops * hop_in] through ``sr`` (in ``slots``, default all), ``groups`` hops per call in turn -> [n, ..] on the host"""
    slots = list(range(sr.S)) if slots is None else slots
    active = None if len(slots) == sr.S else [s in slots for s in range(sr.S)]
    ys, h = [], 0
    for g in groups:
        X = np.zeros((sr.S, g * sr.hop_in), dtype=np.float32)
        X[slots] = x[:, h * sr.hop_in:(h + g) * sr.hop_in]
        buf = torch.full((sr.S, g * sr.hop_out), SENTINEL, device='cuda') if out else None
        y = sr.process(torch.from_numpy(X), active=active, out=buf)
        assert buf is None or y is buf
        ys.append(y.cpu().numpy()[slots])
        h += g
    assert h * sr.hop_in == x.shape[1]
    return np.concatenate(ys, axis=1)


def run(sr_in, sr_out, quality):
    """(x, emitted [B, HOPS * hop_out], flushed [B, D], converter) of the case: one GPU run in calls of (2, 3) hops, shared, never changed"""
    key = (sr_in, sr_out, quality)
    if key not in _RUNS:
        x = _signal(sr_in, sr_out, quality)
        sr = _sr(B, sr_in, sr_out, quality)
        y = feed(sr, x, (2, 3))
        assert (sr.hops == HOPS).all()
        tail = sr.flush(range(B)).cpu().numpy()
        assert (sr.hops == 0).all()
        _RUNS[key] = (x, y, tail, sr)
    return _RUNS[key]


# ------------------------------------------------------------------------------------------------- 1. the offline kernel, delayed by D
@pytest.mark.parametrize('sr_in,sr_out,quality', CASES)
def test_bit_identical_to_the_offline_resampler(sr_in, sr_out, quality):
    from nele_gan_amd.resample import Resampler
    x, y, tail, sr = run(sr_in, sr_out, quality)
    D, n = sr.delay, HOPS * sr.hop_out
    assert y.shape == (B, n) and tail.shape == (B, D)
    whole, n_out = Resampler(sr_in, sr_out, quality).apply(torch.from_numpy(x).cuda(), [x.shape[1]] * B)
    whole = whole.cpu().numpy()
    assert (n_out.cpu().numpy() == n).all() and whole.shape[1] >= n
    assert np.array_equal(y[:, D:].view(np.uint32), whole[:, :n - D].view(np.uint32))
    assert np.array_equal(tail.view(np.uint32), whole[:, n - D:n].view(np.uint32))
    assert np.abs(y[:, :D]).max() > 0.0


# ------------------------------------------------------------------------------------------------- 2. float64
@pytest.mark.parametrize('sr_in,sr_out,quality', CASES)
def test_against_the_float64_reference(sr_in, sr_out, quality):
    from nele_gan_amd.resample import taps
    x, y, tail, sr = run(sr_in, sr_out, quality)
    h = taps(sr.up, sr.down, sr.zeros, sr.beta)
    worst = 0.0
    for b in range(B):
        ref = S.StreamRef(sr.up, sr.down, h, sr.hop_in)
        assert (ref.D, ref.K, ref.n_out) == (sr.delay, sr.K, sr.hop_out)
        y64 = np.concatenate([ref.run(x[b]), ref.flush()])
        got = np.concatenate([y[b], tail[b]]).astype(np.float64)
        ratio = float((np.abs(got - y64) / R.bound(y64, float(np.abs(x[b]).max()))).max())
        worst = max(worst, ratio)
    print('%d -> %d %s: largest |gpu - float64| / bound = %.3f' % (sr_in, sr_out, quality, worst))
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------- 3. grouping and batch
@pytest.mark.parametrize('sr_in,sr_out,quality', [(48000, 16000, 'high'), (12000, 16000, 'high'), (16000, 24000, 'scipy'), (16000, 48000, 'high'),
                                                  (8000, 16000, 'scipy')])
def test_hop_grouping_batch_and_out_buffer_do_not_change_a_slot(sr_in, sr_out, quality):
    x, y, _, _ = run(sr_in, sr_out, quality)                  # calls of (2, 3) hops
    assert np.array_equal(feed(_sr(B, sr_in, sr_out, quality), x, (1,) * HOPS), y)
    assert np.array_equal(feed(_sr(B, sr_in, sr_out, quality), x, (HOPS,)), y)
    assert np.array_equal(feed(_sr(B, sr_in, sr_out, quality), x, (3, 2), out=True), y)
    for row in range(B):
        alone = feed(_sr(1, sr_in, sr_out, quality), x[row:row + 1], (4, 1))
        assert np.array_equal(alone[0], y[row])
    five = _sr(5, sr_in, sr_out, quality)
    others = _signal(sr_in, sr_out, quality, rows=5)[::-1].copy()
    others[3] = x[2]
    assert np.array_equal(feed(five, others, (1, 4))[3], y[2])


# ------------------------------------------------------------------------------------------------- 4. slots
def _record(sr, slot):
    from nele_gan_amd import _lib
    rec = int(_lib.lib.nele_resample_stream_record_bytes(sr.K))
    header = sr.nbytes - sr.S * rec
    assert header == 256
    return sr.state[header + slot * rec:header + (slot + 1) * rec].clone()


@pytest.mark.parametrize('sr_in,sr_out', [(48000, 16000), (16000, 48000)])
def test_inactive_slots_are_neither_read_nor_written(sr_in, sr_out):
    x, y, _, _ = run(sr_in, sr_out, 'high')
    sr = _sr(B, sr_in, sr_out)
    n0, n1 = 2, 2
    feed(sr, x[:, :n0 * sr.hop_in], (n0,))
    before = _record(sr, 1)
    assert before.any()
    X = x[:, n0 * sr.hop_in:(n0 + n1) * sr.hop_in].copy()
    X[1] = np.nan
    out = torch.full((B, n1 * sr.hop_out), SENTINEL, device='cuda')
    sr.process(torch.from_numpy(X), active=[True, False, True], out=out)
    assert (out[1] == SENTINEL).all() and not (out[0] == SENTINEL).any() and not (out[2] == SENTINEL).any()
    assert torch.equal(_record(sr, 1), before)
    assert np.array_equal(out.cpu().numpy()[[0, 2]], y[[0, 2], n0 * sr.hop_out:(n0 + n1) * sr.hop_out])
    # slot 1 goes on where it was: equal to a run that never saw the skipped call
    rest = feed(sr, x[1:2, n0 * sr.hop_in:], (1, 2), slots=[1])
    assert np.array_equal(rest[0], y[1, n0 * sr.hop_out:])


@pytest.mark.parametrize('sr_in,sr_out', [(48000, 16000), (16000, 48000)])
def test_reset_restarts_one_slot_and_leaves_the_others(sr_in, sr_out):
    x, y, _, _ = run(sr_in, sr_out, 'high')
    sr = _sr(B, sr_in, sr_out)
    n0 = 2
    feed(sr, x[:, :n0 * sr.hop_in], (n0,))
    sr.reset([1])
    assert not _record(sr, 1).any() and _record(sr, 0).any() and _record(sr, 2).any()
    assert sr.hops.tolist() == [n0, 0, n0]
    x2 = x[:, n0 * sr.hop_in:].copy()
    x2[1] = x[1, :(HOPS - n0) * sr.hop_in]                    # slot 1 starts its signal again
    got = feed(sr, x2, (1, 2))
    assert np.array_equal(got[1], y[1, :(HOPS - n0) * sr.hop_out])            # as a fresh converter
    assert np.array_equal(got[[0, 2]], y[[0, 2], n0 * sr.hop_out:])           # the neighbours never noticed


# ------------------------------------------------------------------------------------------------- 5. a closed form
@pytest.mark.parametrize('sr_in,sr_out', [(48000, 16000), (8000, 16000)])
def test_a_sinusoid_comes_out_as_that_sinusoid_shifted_by_D(sr_in, sr_out):
    hops, f = 32, 1000.0
    sr = _sr(1, sr_in, sr_out)
    x = np.sin(2.0 * np.pi * f * np.arange(hops * sr.hop_in) / sr_in).astype(np.float32)
    y = feed(sr, x[None], (7, 25))[0].astype(np.float64)
    m = np.arange(len(y))
    want = np.sin(2.0 * np.pi * f * (m - sr.delay) / sr_out)
    skip = 72 + sr.delay
    err = float(np.abs(y - want)[skip:].max())
    print('%d -> %d: 1 kHz sinusoid, largest error behind output %d: %.3g' % (sr_in, sr_out, skip, err))
    assert err <= 1e-5


# ------------------------------------------------------------------------------------------------- 6. RateAdaptedEnhancer
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


def _device_signals(rate, streams, hops, impulse_at):
    """clean: a low Gaussian floor with one unit impulse per row; second: Gaussian noise; float32 at the device rate"""
    hop = rate * S.HOP // S.RATE
    rs = np.random.RandomState(rate // 1000)
    clean = (1e-3 * rs.randn(streams, hops * hop)).astype(np.float32)
    for b, t in enumerate(impulse_at):
        clean[b, t] = 1.0
    second = (0.05 * rs.randn(streams, hops * hop)).astype(np.float32)
    return clean, second, hop


@pytest.mark.parametrize('rate', [48000, 8000])
def test_rate_adapted_enhancer_is_the_chain_by_hand(rate):
    """B = 2, 6 hops in calls of (1, 2, 3) and drain.  By hand: a StreamResampler down on each signal, RealtimeEnhancer.process hop by
    hop, a StreamResampler up.  The impulse of each row comes out ``latency`` samples later: the peak of |out| marks the middle of the
    nonzero region an impulse leaves (both filters are symmetric and the 16 kHz grid holds the impulse's place: it sits on a multiple
    of the decimation factor), and its expected place is put together here from the converters' delays and the hops."""
    from nele_gan_amd.streamrate import RateAdaptedEnhancer
    Bw, hops = 2, 6
    G = _generator()
    hop = rate * S.HOP // S.RATE
    step = max(1, rate // S.RATE)
    t0 = [hop + 100 * step, 2 * hop + 33 * step]
    clean, second, hop = _device_signals(rate, Bw, hops, t0)
    wrap = RateAdaptedEnhancer(_rt(G, Bw), rate)
    assert wrap.hop == hop and wrap.down.S == 2 * Bw and wrap.up.S == Bw
    outs, h = [], 0
    for g in (1, 2, 3):
        outs.append(wrap.process(torch.from_numpy(clean[:, h * hop:(h + g) * hop]), torch.from_numpy(second[:, h * hop:(h + g) * hop])))
        h += g
    outs.append(wrap.drain(range(Bw)))
    got = torch.cat(outs, dim=1).cpu().numpy()
    nd = -(-wrap.latency // hop)
    assert got.shape == (Bw, (hops + nd) * hop)
    # ---- by hand
    dc, dn, rt, up = _sr(Bw, rate, S.RATE), _sr(Bw, rate, S.RATE), _rt(G, Bw), _sr(Bw, S.RATE, rate)
    zc = np.concatenate([clean, np.zeros((Bw, nd * hop), np.float32)], axis=1)
    zs = np.concatenate([second, np.zeros((Bw, nd * hop), np.float32)], axis=1)
    hand = []
    for k in range(hops + nd):
        c16 = dc.process(torch.from_numpy(zc[:, k * hop:(k + 1) * hop]))
        n16 = dn.process(torch.from_numpy(zs[:, k * hop:(k + 1) * hop]))
        hand.append(up.process(rt.process(c16, n16)))
    hand = torch.cat(hand, dim=1).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), hand.view(np.uint32))
    # ---- latency: D_down at 16 kHz in device samples, the enhancer's hop, D_up
    expected = dc.delay * hop // S.HOP + hop + up.delay
    assert wrap.latency == expected
    assert expected == {48000: 960, 8000: 192}[rate]          # 20 ms / 24 ms (section 15)
    for b in range(Bw):
        peak = int(np.abs(got[b]).argmax())
        print('%d Hz row %d: impulse at %d, peak of |out| at %d, latency %d' % (rate, b, t0[b], peak, wrap.latency))
        assert peak - t0[b] == expected
    # ---- reset: the wrapper starts again as a new one
    wrap.reset(range(Bw))
    again = wrap.process(torch.from_numpy(clean[:, :hop]), torch.from_numpy(second[:, :hop])).cpu().numpy()
    assert np.array_equal(again.view(np.uint32), got[:, :hop].view(np.uint32))


def test_rate_adapted_enhancer_around_the_echo_canceller():
    """48 kHz, P = 2, 2 hops per call: the wrapper around an EchoCancellingEnhancer against the converters and a second loop by hand"""
    from nele_gan_amd.aec import EchoCanceller, EchoCancellingEnhancer
    from nele_gan_amd.streamrate import RateAdaptedEnhancer
    Bw, hops, rate = 2, 6, 48000
    G = _generator()
    clean, mic, hop = _device_signals(rate, Bw, hops, [900, 1700])
    wrap = RateAdaptedEnhancer(EchoCancellingEnhancer(_rt(G, Bw), EchoCanceller(Bw, partitions=2)), rate)
    loop = EchoCancellingEnhancer(_rt(G, Bw), EchoCanceller(Bw, partitions=2))
    dc, dm, up = _sr(Bw, rate, S.RATE), _sr(Bw, rate, S.RATE), _sr(Bw, S.RATE, rate)
    got, hand = [], []
    for k in range(0, hops, 2):
        c, m = torch.from_numpy(clean[:, k * hop:(k + 2) * hop]), torch.from_numpy(mic[:, k * hop:(k + 2) * hop])
        got.append(wrap.process(c, m))
        hand.append(up.process(loop.process(dc.process(c), dm.process(m))))
    got.append(wrap.drain([0, 1]))
    z = torch.zeros((Bw, 2 * hop))
    hand.append(up.process(loop.process(dc.process(z), dm.process(z))))
    got, hand = torch.cat(got, dim=1).cpu().numpy(), torch.cat(hand, dim=1).cpu().numpy()
    assert got.shape == hand.shape == (Bw, (hops + 2) * hop)
    assert np.array_equal(got.view(np.uint32), hand.view(np.uint32))
    assert np.isfinite(got).all() and np.abs(got).max() > 0.0


def test_rate_adapted_enhancer_at_16_khz_is_the_inner_object():
    from nele_gan_amd.streamrate import RateAdaptedEnhancer
    Bw, hops = 2, 3
    G = _generator()
    clean, noise, hop = _device_signals(S.RATE, Bw, hops, [300, 500])
    wrap, rt = RateAdaptedEnhancer(_rt(G, Bw), S.RATE), _rt(G, Bw)
    assert wrap.down is None and wrap.up is None and wrap.hop == S.HOP and wrap.latency == S.HOP
    a = wrap.process(torch.from_numpy(clean), torch.from_numpy(noise)).cpu().numpy()
    b = rt.process(torch.from_numpy(clean), torch.from_numpy(noise)).cpu().numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------- 7. errors
def test_errors_are_value_errors_before_any_launch():
    from nele_gan_amd.streamrate import RateAdaptedEnhancer
    sr = _sr(B, 48000, 16000)
    before = sr.state.clone()
    good = torch.zeros((B, 768))
    with pytest.raises(ValueError, match='x must be'):
        sr.process(torch.zeros((B, 767)))
    with pytest.raises(ValueError, match='x must be'):
        sr.process(torch.zeros((B + 1, 768)))
    with pytest.raises(ValueError, match='x must be float32'):
        sr.process(torch.zeros((B, 768), dtype=torch.float64))
    with pytest.raises(ValueError, match='active'):
        sr.process(good, active=[True] * (B + 1))
    with pytest.raises(ValueError, match='out must be'):
        sr.process(good, out=torch.zeros((B, 255), device='cuda'))
    with pytest.raises(ValueError, match='out must be'):
        sr.process(good, out=torch.zeros((B, 256), dtype=torch.float64, device='cuda'))
    with pytest.raises(ValueError, match='44.1 kHz'):
        _sr(B, 44100, 16000)
    assert torch.equal(sr.state, before) and not sr.hops.any()
    with pytest.raises(ValueError, match='inner'):
        RateAdaptedEnhancer(sr, 48000)
    rt = _rt(_generator(), 2)
    with pytest.raises(ValueError, match='44.1 kHz'):
        RateAdaptedEnhancer(rt, 44100)
    wrap = RateAdaptedEnhancer(rt, 48000)
    ok = torch.zeros((2, 768))
    with pytest.raises(ValueError, match='clean must be'):
        wrap.process(torch.zeros((2, 256)), torch.zeros((2, 256)))
    with pytest.raises(ValueError, match='second must be'):
        wrap.process(ok, torch.zeros((2, 1536)))
    with pytest.raises(ValueError, match='second must be float32'):
        wrap.process(ok, ok.double())
    with pytest.raises(ValueError, match='active'):
        wrap.process(ok, ok, active=[True])
    assert not wrap.down.hops.any() and not wrap.up.hops.any() and not rt.hops.any()
