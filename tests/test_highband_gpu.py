"""GPU: the up-converter that carries the band above 8 kHz (nele_gan_amd/highband.py HighBandUp, csrc/highband.hip) and
RateAdaptedEnhancer(.., highband=..) (nele_gan_amd/streamrate.py) against DESIGN.md section 24: the composition built from the existing
stream converter and float32 torch ops on the host (bitwise for g = 1, 0.5, 0), tests/highband_ref.py with the specification's float32
roundings (g = 0.7), the identity, the streaming contract (grouping, batch, slots, reset: bitwise), the wrapper against the chain built
by hand (bitwise), an 18 kHz tone through the whole wrapper, and an impulse.

Bounds.  Composition: equal bits - g low and g x are exact products for g = 1, 0.5, 0, so fmaf(-g, low, enh) and fmaf(g, x, u) are the
correctly rounded difference and sum torch computes.  g = 0.7: resample_ref.bound per sample (one float32 ulp of the result plus
1e-12 max |d|, the converter's own bound) plus one float32 ulp of g x.  Tone: 1e-5, section 15's sinusoid bound (the float64 reference
gives 2e-14; 18 kHz is 1.96 x above the stop-band edge of 1.15 x 8 kHz).
Measured on an MI355X: bit-equal to the composition in all 21 cases (3 rates, 2 lags and 96 kHz with lag_hops 3, 3 gains); g = 0.7: largest
|gpu - reference| / bound 0.000 in all seven cases (every sample bit-equal to the reference with the specification's roundings); 18 kHz tone in phase
1.000000527 / 1.000000462 with the band (quadrature <= 3.4e-7), 0.500000523 / 0.500000458 at g = 0.5, 5.2e-7 / 4.6e-7 left without it;
impulse peaks exactly ``latency`` late (1068 -> 2028, 1635 -> 2595; lag_hops 2: 1068 -> 2796, 1635 -> 3363), with the band and for the
low band alone through the same inner objects; the whole file runs in 3 s."""
import numpy as np
import pytest

import highband_ref as HB
import resample_ref as R
import streamrate_ref as S

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from weights_recipe import seeded_state_arrays  # noqa: E402

B, HOPS, SENTINEL = 3, 5, -7.25
# 96 kHz with lag_hops 3: a record of 5824 floats, above the 4096 the staging space holds - it moves in two chunks
CASES = [(rate, lag) for rate in (48000, 24000, 96000) for lag in (1, 2)] + [(96000, 3)]
_RUNS = {}


def _hb(streams, rate, lag_hops=1, g=None):
    from nele_gan_amd.highband import HighBandUp
    hb = HighBandUp(streams, rate, lag_hops)
    if g is not None:
        hb.gain.fill_(g)
    return hb


def _signals(rate, lag_hops, rows=B, hops=HOPS):
    """(enh, low, x): float32 Gaussian rows without a zero sample, row 1 scaled by 1e-6 and row 2 by 1e3"""
    N = rate * S.HOP // S.RATE
    rs = np.random.RandomState(rate // 1000 + lag_hops + rows)
    out = []
    for width in (hops * S.HOP, hops * S.HOP, hops * N):
        v = rs.randn(rows, width).astype(np.float32)
        v[v == 0.0] = 1.0
        if rows > 1:
            v[1] *= np.float32(1e-6)
        if rows > 2:
            v[2] *= np.float32(1e3)
        out.append(v)
    return out


def _delayed(v, n):
    """rows of v behind n zeros, cut to v's width (numpy or torch)"""
    if isinstance(v, np.ndarray):
        return np.concatenate([np.zeros((v.shape[0], n), v.dtype), v], axis=1)[:, :v.shape[1]]
    return torch.cat([torch.zeros((v.shape[0], n), dtype=v.dtype), v], dim=1)[:, :v.shape[1]]


def feed(hb, enh, low, x, groups, slots=None, out=False):
    """the columns of the three signals through ``hb`` (in ``slots``, default all), ``groups`` hops per call in turn -> [n, ..] on the host"""
    slots = list(range(hb.S)) if slots is None else slots
    active = None if len(slots) == hb.S else [s in slots for s in range(hb.S)]
    N, ys, h = hb.hop_out, [], 0
    for g in groups:
        E, Lo, X = (np.zeros((hb.S, g * w), dtype=np.float32) for w in (S.HOP, S.HOP, N))
        E[slots], Lo[slots], X[slots] = enh[:, h * S.HOP:(h + g) * S.HOP], low[:, h * S.HOP:(h + g) * S.HOP], x[:, h * N:(h + g) * N]
        buf = torch.full((hb.S, g * N), SENTINEL, device='cuda') if out else None
        y = hb.process(torch.from_numpy(E).cuda(), torch.from_numpy(Lo).cuda(), torch.from_numpy(X).cuda(), active=active, out=buf)
        assert buf is None or y is buf
        ys.append(y.cpu().numpy()[slots])
        h += g
    assert h * N == x.shape[1]
    return np.concatenate(ys, axis=1)


def run(rate, lag_hops, g=1.0):
    """(enh, low, x, y [B, HOPS * N]) of the case: one GPU run in calls of (2, 3) hops, shared, never changed"""
    key = (rate, lag_hops, g)
    if key not in _RUNS:
        enh, low, x = _signals(rate, lag_hops)
        hb = _hb(B, rate, lag_hops, g)
        y = feed(hb, enh, low, x, (2, 3))
        assert (hb.hops == HOPS).all()
        _RUNS[key] = (enh, low, x, y)
    return _RUNS[key]


def composed(rate, lag_hops, g, enh, low, x, groups=(2, 3)):
    """StreamResampler(16 kHz -> rate).process(enh - g low delayed) + g x delayed: subtraction, delays and addition in float32 torch on
    the host -> numpy [rows, ..]"""
    from nele_gan_amd.highband import highband_plan
    from nele_gan_amd.resample import StreamResampler
    plan = highband_plan(rate, lag_hops)
    e, lo, xx = torch.from_numpy(enh), torch.from_numpy(low), torch.from_numpy(x)
    gt = torch.tensor(g, dtype=torch.float32)
    d = e - gt * _delayed(lo, plan['lag16'])
    up = StreamResampler(enh.shape[0], S.RATE, rate)
    us, h = [], 0
    for k in groups:
        us.append(up.process(d[:, h * S.HOP:(h + k) * S.HOP].contiguous()).cpu())
        h += k
    y = torch.cat(us, dim=1) + gt * _delayed(xx, plan['lag'])
    assert y.dtype == torch.float32
    return y.numpy()


# ------------------------------------------------------------------------------------------------- 1. the composition
@pytest.mark.parametrize('rate,lag_hops', CASES)
def test_bit_identical_to_the_composition_for_exact_gains(rate, lag_hops):
    for g in (1.0, 0.5, 0.0):
        enh, low, x, y = run(rate, lag_hops, g)
        want = composed(rate, lag_hops, g, enh, low, x)
        assert y.shape == want.shape == (B, HOPS * rate * S.HOP // S.RATE)
        assert np.array_equal(y.view(np.uint32), want.view(np.uint32)), g
    assert not np.array_equal(run(rate, lag_hops, 1.0)[3], run(rate, lag_hops, 0.5)[3])


@pytest.mark.parametrize('rate,lag_hops', CASES)
def test_an_inexact_gain_against_the_reference(rate, lag_hops):
    g = 0.7
    enh, low, x, y = run(rate, lag_hops, g)
    g32 = np.float32(g)
    worst = 0.0
    for b in range(B):
        ref = HB.HighBandRef(rate, lag_hops, g=g, rounded=True)
        y64 = ref.process(enh[b], low[b], x[b])
        dmax = float(np.abs(enh[b].astype(np.float64) - float(g32) * _delayed(low[b:b + 1], ref.lam)[0]).max())
        gx = (g32 * _delayed(x[b:b + 1], ref.L)[0]).astype(np.float32)
        bound = R.bound(y64, dmax) + np.spacing(np.abs(gx)).astype(np.float64)
        worst = max(worst, float((np.abs(y[b].astype(np.float64) - y64) / bound).max()))
    print('%d Hz, lag_hops %d, g = 0.7: largest |gpu - reference| / bound = %.3f' % (rate, lag_hops, worst))
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------- 2. the identity
@pytest.mark.parametrize('rate,lag_hops', CASES)
def test_an_enhancer_that_changes_nothing_gives_the_bits_of_the_input_delayed_by_L(rate, lag_hops):
    _, low, x = _signals(rate, lag_hops)
    hb = _hb(B, rate, lag_hops)
    enh = _delayed(low, hb.lag16)
    y = feed(hb, enh, low, x, (1, 1, 1, 1, 1))
    assert np.array_equal(y.view(np.uint32), _delayed(x, hb.lag).view(np.uint32))
    assert not (x == 0.0).any() and hb.lag > hb.hop_out                      # x[m - L] reaches two hops back


# ------------------------------------------------------------------------------------------------- 3. grouping and batch
@pytest.mark.parametrize('rate,lag_hops', CASES)
def test_hop_grouping_batch_and_out_buffer_do_not_change_a_slot(rate, lag_hops):
    enh, low, x, y = run(rate, lag_hops)                     # calls of (2, 3) hops
    assert np.array_equal(feed(_hb(B, rate, lag_hops), enh, low, x, (1,) * HOPS), y)
    assert np.array_equal(feed(_hb(B, rate, lag_hops), enh, low, x, (HOPS,)), y)
    assert np.array_equal(feed(_hb(B, rate, lag_hops), enh, low, x, (3, 2), out=True), y)
    alone = feed(_hb(1, rate, lag_hops), enh[2:3], low[2:3], x[2:3], (4, 1))
    assert np.array_equal(alone[0], y[2])
    five = _hb(5, rate, lag_hops)
    others = [v[::-1].copy() for v in _signals(rate, lag_hops, rows=5)]
    for v, mine in zip(others, (enh, low, x)):
        v[2] = mine[2]
    assert np.array_equal(feed(five, *others, (1, 4))[2], y[2])


def test_rows_of_wider_tensors_pass_without_a_copy():
    """low as rows 0 .. B - 1 of a [2 B, ..] tensor, x likewise, enh and out with their own strides checked"""
    enh, low, x, y = run(48000, 1)
    hb = _hb(B, 48000)
    both16 = torch.full((2 * B, HOPS * S.HOP), float('nan'), device='cuda')
    both48 = torch.full((2 * B, HOPS * 768), float('nan'), device='cuda')
    both16[:B], both48[:B] = torch.from_numpy(low).cuda(), torch.from_numpy(x).cuda()
    wide = torch.full((B, HOPS * S.HOP + 64), float('nan'), device='cuda')
    wide[:, :HOPS * S.HOP] = torch.from_numpy(enh).cuda()
    got = hb.process(wide[:, :HOPS * S.HOP], both16[:B], both48[:B]).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), y.view(np.uint32))
    with pytest.raises(ValueError, match='low16 must be'):
        hb.process(wide[:, :HOPS * S.HOP], torch.zeros((HOPS * S.HOP, B), device='cuda').t(), both48[:B])       # the shape, but columns B apart
    with pytest.raises(ValueError, match='x_dev must be'):
        hb.process(wide[:, :HOPS * S.HOP], both16[:B], both48[:B].cpu())
    with pytest.raises(ValueError, match='out must be'):
        hb.process(wide[:, :HOPS * S.HOP], both16[:B], both48[:B], out=torch.zeros((B, 767), device='cuda'))
    assert (hb.hops == HOPS).all()


# ------------------------------------------------------------------------------------------------- 4. slots
def _record(hb, slot):
    from nele_gan_amd import _lib
    rec = int(_lib.lib.nele_hbup_record_bytes(hb.K, hb.lag16, hb.lag))
    header = hb.nbytes - hb.S * rec
    assert header == 256 and rec == (4 * (hb.K - 1 + hb.lag16 + hb.lag) + 255) // 256 * 256
    return hb.state[header + slot * rec:header + (slot + 1) * rec].clone()


@pytest.mark.parametrize('rate,lag_hops', [(48000, 1), (24000, 2)])
def test_inactive_slots_are_neither_read_nor_written(rate, lag_hops):
    enh, low, x, y = run(rate, lag_hops)
    hb = _hb(B, rate, lag_hops)
    N, n0, n1 = hb.hop_out, 2, 2
    feed(hb, enh[:, :n0 * S.HOP], low[:, :n0 * S.HOP], x[:, :n0 * N], (n0,))
    before = _record(hb, 1)
    assert before.any()
    part = [v[:, n0 * w:(n0 + n1) * w].copy() for v, w in ((enh, S.HOP), (low, S.HOP), (x, N))]
    for v in part:
        v[1] = np.nan
    out = torch.full((B, n1 * N), SENTINEL, device='cuda')
    hb.process(*(torch.from_numpy(v).cuda() for v in part), active=[True, False, True], out=out)
    assert (out[1] == SENTINEL).all() and not (out[0] == SENTINEL).any() and not (out[2] == SENTINEL).any()
    assert torch.equal(_record(hb, 1), before)
    assert np.array_equal(out.cpu().numpy()[[0, 2]], y[[0, 2], n0 * N:(n0 + n1) * N])
    # slot 1 goes on where it was: equal to a run that never saw the skipped call
    rest = feed(hb, enh[1:2, n0 * S.HOP:], low[1:2, n0 * S.HOP:], x[1:2, n0 * N:], (1, 2), slots=[1])
    assert np.array_equal(rest[0], y[1, n0 * N:])


@pytest.mark.parametrize('rate,lag_hops', [(48000, 1), (96000, 2)])
def test_reset_restarts_one_slot_and_leaves_the_others(rate, lag_hops):
    enh, low, x, y = run(rate, lag_hops)
    hb = _hb(B, rate, lag_hops)
    N, n0 = hb.hop_out, 2
    feed(hb, enh[:, :n0 * S.HOP], low[:, :n0 * S.HOP], x[:, :n0 * N], (n0,))
    hb.reset([1])
    assert not _record(hb, 1).any() and _record(hb, 0).any() and _record(hb, 2).any()
    assert hb.hops.tolist() == [n0, 0, n0]
    e2, l2, x2 = enh[:, n0 * S.HOP:].copy(), low[:, n0 * S.HOP:].copy(), x[:, n0 * N:].copy()
    e2[1], l2[1], x2[1] = enh[1, :(HOPS - n0) * S.HOP], low[1, :(HOPS - n0) * S.HOP], x[1, :(HOPS - n0) * N]     # slot 1 starts again
    got = feed(hb, e2, l2, x2, (1, 2))
    assert np.array_equal(got[1], y[1, :(HOPS - n0) * N])                    # as a fresh object
    assert np.array_equal(got[[0, 2]], y[[0, 2], n0 * N:])                   # the neighbours never noticed


# ------------------------------------------------------------------------------------------------- 5. the wrapper by hand
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
    from nele_gan_amd.resample import StreamResampler
    return StreamResampler(streams, sr_in, sr_out)


def _device_signals(rate, streams, hops, impulse_at):
    """clean: a low Gaussian floor with one unit impulse per row; second: Gaussian noise; float32 at the device rate"""
    hop = rate * S.HOP // S.RATE
    rs = np.random.RandomState(rate // 1000)
    clean = (1e-3 * rs.randn(streams, hops * hop)).astype(np.float32)
    for b, t in enumerate(impulse_at):
        clean[b, t] = 1.0
    second = (0.05 * rs.randn(streams, hops * hop)).astype(np.float32)
    return clean, second, hop


def _by_hand(up, lam_hist, x_hist, enh, low, x):
    """item 1's composition for one call, the two delay lines kept by the caller as host tensors (updated in place)"""
    lows, xs = torch.cat([lam_hist[0], low.cpu()], dim=1), torch.cat([x_hist[0], x], dim=1)
    lam_hist[0], x_hist[0] = lows[:, low.shape[1]:], xs[:, x.shape[1]:]
    d = enh.cpu() - lows[:, :low.shape[1]]
    return up.process(d.contiguous()).cpu() + xs[:, :x.shape[1]]


def test_rate_adapted_enhancer_with_the_band_is_the_chain_by_hand():
    """B = 2, 6 hops at 48 kHz in calls of (1, 2, 3) and drain.  By hand: a StreamResampler down on each signal, RealtimeEnhancer.process
    hop by hop, then StreamResampler up of enh - low delayed, plus clean delayed, in float32 torch on the host."""
    from nele_gan_amd.streamrate import RateAdaptedEnhancer
    Bw, hops, rate = 2, 6, 48000
    G = _generator()
    clean, second, hop = _device_signals(rate, Bw, hops, [1068, 1899])
    wrap = RateAdaptedEnhancer(_rt(G, Bw), rate, highband=True)
    assert wrap.hop == hop and wrap.latency == wrap.up.lag == 960 and wrap.up.lag_hops == 1 and wrap.down.S == 2 * Bw and wrap.up.S == Bw
    outs, h = [], 0
    for g in (1, 2, 3):
        outs.append(wrap.process(torch.from_numpy(clean[:, h * hop:(h + g) * hop]), torch.from_numpy(second[:, h * hop:(h + g) * hop])))
        h += g
    outs.append(wrap.drain(range(Bw)))
    got = torch.cat(outs, dim=1).cpu().numpy()
    nd = -(-wrap.latency // hop)
    assert got.shape == (Bw, (hops + nd) * hop)
    dc, dn, rt, up = _sr(Bw, rate, S.RATE), _sr(Bw, rate, S.RATE), _rt(G, Bw), _sr(Bw, S.RATE, rate)
    zc = np.concatenate([clean, np.zeros((Bw, nd * hop), np.float32)], axis=1)
    zs = np.concatenate([second, np.zeros((Bw, nd * hop), np.float32)], axis=1)
    lam_hist, x_hist, hand = [torch.zeros((Bw, 256))], [torch.zeros((Bw, 960))], []
    for k in range(hops + nd):
        xk = torch.from_numpy(zc[:, k * hop:(k + 1) * hop])
        c16 = dc.process(xk)
        n16 = dn.process(torch.from_numpy(zs[:, k * hop:(k + 1) * hop]))
        hand.append(_by_hand(up, lam_hist, x_hist, rt.process(c16, n16), c16, xk))
    hand = torch.cat(hand, dim=1).numpy()
    assert np.array_equal(got.view(np.uint32), hand.view(np.uint32))
    # reset: the wrapper starts again as a new one
    wrap.reset(range(Bw))
    again = wrap.process(torch.from_numpy(clean[:, :hop]), torch.from_numpy(second[:, :hop])).cpu().numpy()
    assert np.array_equal(again.view(np.uint32), got[:, :hop].view(np.uint32))


def test_rate_adapted_enhancer_with_the_band_around_the_echo_canceller():
    """48 kHz, P = 2, 2 hops per call: the wrapper around an EchoCancellingEnhancer against the converters and a second loop by hand"""
    from nele_gan_amd.aec import EchoCanceller, EchoCancellingEnhancer
    from nele_gan_amd.streamrate import RateAdaptedEnhancer
    Bw, hops, rate = 2, 6, 48000
    G = _generator()
    clean, mic, hop = _device_signals(rate, Bw, hops, [900, 1700])
    wrap = RateAdaptedEnhancer(EchoCancellingEnhancer(_rt(G, Bw), EchoCanceller(Bw, partitions=2)), rate, highband=True)
    assert wrap.latency == 960
    loop = EchoCancellingEnhancer(_rt(G, Bw), EchoCanceller(Bw, partitions=2))
    dc, dm, up = _sr(Bw, rate, S.RATE), _sr(Bw, rate, S.RATE), _sr(Bw, S.RATE, rate)
    lam_hist, x_hist, got, hand = [torch.zeros((Bw, 256))], [torch.zeros((Bw, 960))], [], []
    z = torch.zeros((Bw, 2 * hop))
    for k in range(0, hops + 2, 2):
        c, m = (torch.from_numpy(clean[:, k * hop:(k + 2) * hop]), torch.from_numpy(mic[:, k * hop:(k + 2) * hop])) if k < hops else (z, z)
        got.append(wrap.process(c, m) if k < hops else wrap.drain([0, 1]))
        c16 = dc.process(c)
        hand.append(_by_hand(up, lam_hist, x_hist, loop.process(c16, dm.process(m)), c16, c))
    got, hand = torch.cat(got, dim=1).cpu().numpy(), torch.cat(hand, dim=1).numpy()
    assert got.shape == hand.shape == (Bw, (hops + 2) * hop)
    assert np.array_equal(got.view(np.uint32), hand.view(np.uint32))
    assert np.isfinite(got).all() and np.abs(got).max() > 0.0


def test_without_the_keyword_the_wrapper_is_what_it_was():
    """highband=None: the down-converter, the enhancer and the plain up-converter, bit for bit, and the latency arithmetic of before"""
    from nele_gan_amd.resample import StreamResampler
    from nele_gan_amd.streamrate import RateAdaptedEnhancer, adapt
    Bw, hops, rate = 2, 4, 48000
    G = _generator()
    clean, second, hop = _device_signals(rate, Bw, hops, [800, 1700])
    wrap, via = RateAdaptedEnhancer(_rt(G, Bw), rate), adapt(_rt(G, Bw), rate, highband=None)
    assert type(wrap.up) is StreamResampler and type(via.up) is StreamResampler and wrap.highband is None and wrap.latency == via.latency == 960
    dc, dn, rt, up = _sr(Bw, rate, S.RATE), _sr(Bw, rate, S.RATE), _rt(G, Bw), _sr(Bw, S.RATE, rate)
    c, s = torch.from_numpy(clean), torch.from_numpy(second)
    hand = up.process(rt.process(dc.process(c), dn.process(s))).cpu().numpy()
    for w in (wrap, via):
        assert np.array_equal(w.process(c, s).cpu().numpy().view(np.uint32), hand.view(np.uint32))


# ------------------------------------------------------------------------------------------------- 6. the point of it
def test_an_18_khz_tone_passes_the_wrapper_only_with_the_band():
    """B = 2, 32 hops at 48 kHz: clean = a unit 18 kHz sinusoid + 0.5 of a 1 kHz one, noise a 1e-3 Gaussian floor.  The output is
    projected onto the 18 kHz sinusoid delayed by ``latency`` over hops 8 .. 31: 18432 samples, 6912 and 384 periods."""
    from nele_gan_amd.streamrate import RateAdaptedEnhancer
    Bw, hops, rate, f = 2, 32, 48000, 18000.0
    G = _generator()
    hop = 768
    m = np.arange(hops * hop)
    clean = (np.sin(2.0 * np.pi * f * m / rate) + 0.5 * np.sin(2.0 * np.pi * 1000.0 * m / rate)).astype(np.float32)[None].repeat(Bw, axis=0)
    noise = (1e-3 * np.random.RandomState(18).randn(Bw, hops * hop)).astype(np.float32)
    win = slice(8 * hop, hops * hop)
    assert ((hops - 8) * hop * f / rate) % 1.0 == 0.0 and ((hops - 8) * hop * 1000.0 / rate) % 1.0 == 0.0
    amps = {}
    for hbk in (True, None, 0.5):
        wrap = RateAdaptedEnhancer(_rt(G, Bw), rate, highband=hbk)
        assert wrap.latency == 960
        out = torch.cat([wrap.process(torch.from_numpy(clean[:, k * hop:(k + 8) * hop]), torch.from_numpy(noise[:, k * hop:(k + 8) * hop]))
                         for k in range(0, hops, 8)], dim=1).cpu().numpy().astype(np.float64)
        ref_s, ref_c = np.sin(2.0 * np.pi * f * (m - wrap.latency) / rate)[win], np.cos(2.0 * np.pi * f * (m - wrap.latency) / rate)[win]
        amps[hbk] = [(2.0 * np.mean(out[b, win] * ref_s), 2.0 * np.mean(out[b, win] * ref_c)) for b in range(Bw)]
        print('highband=%s: 18 kHz in phase / quadrature per row: %s' % (hbk, ['%.9f / %.3g' % ab for ab in amps[hbk]]))
    for b in range(Bw):
        assert abs(amps[True][b][0] - 1.0) <= 1e-5 and abs(amps[True][b][1]) <= 1e-5
        assert np.hypot(*amps[None][b]) < 1e-5
        assert abs(amps[0.5][b][0] - 0.5) <= 1e-5 and abs(amps[0.5][b][1]) <= 1e-5


# ------------------------------------------------------------------------------------------------- 7. an impulse
@pytest.mark.parametrize('lag_hops', [1, 2])
def test_an_impulse_comes_out_latency_samples_later(lag_hops):
    """48 kHz: a unit impulse in ``clean`` over the floor; lag_hops 2 is an EchoCancellingEnhancer around a CompressedEnhancer.  The peak
    with the band is the carried impulse itself, L late by construction; that L is the low band's own delay through the real inner
    object - that ``lag_hops`` is right for it - shows where the same objects without the band (up(enh) alone) put their peak."""
    from nele_gan_amd.aec import EchoCanceller, EchoCancellingEnhancer
    from nele_gan_amd.drc import CompressedEnhancer, StreamCompressor
    from nele_gan_amd.streamrate import RateAdaptedEnhancer
    Bw, hops, rate = 2, 6, 48000
    G = _generator()
    t0 = [768 + 300, 2 * 768 + 99]
    clean, second, hop = _device_signals(rate, Bw, hops, t0)

    def inner():
        if lag_hops == 1:
            return _rt(G, Bw)
        return EchoCancellingEnhancer(CompressedEnhancer(_rt(G, Bw), StreamCompressor(Bw)), EchoCanceller(Bw, partitions=2))

    def through(w):
        return torch.cat([w.process(torch.from_numpy(clean[:, k * hop:(k + 2) * hop]), torch.from_numpy(second[:, k * hop:(k + 2) * hop]))
                          for k in range(0, hops, 2)], dim=1).cpu().numpy()
    wrap, plain = RateAdaptedEnhancer(inner(), rate, highband=True), RateAdaptedEnhancer(inner(), rate)
    assert wrap.up.lag_hops == lag_hops and wrap.latency == {1: 960, 2: 1728}[lag_hops]
    got, low_only = through(wrap), through(plain)
    peaks = []
    for b in range(Bw):
        peak, peak_low = int(np.abs(got[b]).argmax()), int(np.abs(low_only[b]).argmax())
        print('lag_hops %d row %d: impulse at %d, peak of |out| at %d, of the low band alone at %d, latency %d'
              % (lag_hops, b, t0[b], peak, peak_low, wrap.latency))
        peaks.append((peak - t0[b], peak_low - t0[b]))
    assert peaks == [(wrap.latency, wrap.latency)] * Bw
