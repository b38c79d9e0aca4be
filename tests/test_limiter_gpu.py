"""GPU: the stream limiter (nele_gan_amd/limiter.py, csrc/limiter.hip) against tests/limiter_ref.py - the float64 numpy restatement of
DESIGN.md section 26.  Every operation of the contract is an IEEE basic operation, so out, gain and peak are compared BIT FOR BIT, here
and in the streaming contract (grouping, batch, slots, skipped calls, reset); then LimitedEnhancer around the rule-mode enhancer and the
compressed chain, inside the echo loop, under the 48 kHz wrapper with the high band carried, and the command line.

Measured on an MI355X: out, gain and peak differ from the reference in 0 of their values in every parity shape; on noise at 4 c
max |out| = 0.8994 cf and the clamp does not act; the impulse at 1068 leaves at 3564 with and without the band (latency 2496); the
whole file runs in 4 s."""

import numpy as np
import pytest

import limiter_cases as K
from limiter_ref import CEILING, HOP, LimRef, floor32

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

SENTINEL = -7.25
WANT = ('gain', 'peak')
CF = floor32(CEILING)


def _lim(B, **kw):
    from nele_gan_amd.limiter import StreamLimiter
    return StreamLimiter(B, **kw)


def feed(lim, xs, group, slots=None):
    """all hops of the given streams through ``lim`` (in ``slots``, default 0 ..), ``group`` hops per call at most
    -> dict: out [n, L] float32; gain [n, L], peak [n, L / 256] float64, on the host"""
    slots = list(range(len(xs))) if slots is None else slots
    L = len(xs[0])
    parts = {k: [] for k in ('out',) + WANT}
    for a in range(0, L, group * HOP):
        b = min(L, a + group * HOP)
        X = np.full((lim.S, b - a), np.nan, np.float32)
        act = np.zeros(lim.S, bool)
        for i, s in enumerate(slots):
            X[s], act[s] = xs[i][a:b], True
        got = lim.process(torch.from_numpy(X), active=None if act.all() else act, want=WANT)
        for k, t in zip(('out',) + WANT, got):
            parts[k].append(t[slots].cpu().numpy())
    return {k: np.concatenate(v, axis=1) for k, v in parts.items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same(a, b, rows=slice(None)):
    """the output and the two optional outputs, bit for bit"""
    return all(a[k][rows].shape == b[k].shape and a[k].dtype == b[k].dtype and np.array_equal(bits(a[k][rows]), bits(b[k])) for k in ('out',) + WANT)


def cut(d, rows=slice(None), hops=slice(None)):
    samples = slice(None if hops.start is None else hops.start * HOP, None if hops.stop is None else hops.stop * HOP)
    return {'out': d['out'][rows, samples], 'gain': d['gain'][rows, samples], 'peak': d['peak'][rows, hops]}


def check_parity(tag, got, row, ref):
    for k in ('out',) + WANT:
        differ = int((bits(got[k][row]) != bits(ref[k])).sum())
        print('%s: %s differs from the reference in %d of %d values' % (tag, k, differ, ref[k].size))
    assert got['out'].dtype == np.float32 and got['gain'].dtype == np.float64 and got['peak'].dtype == np.float64
    assert same(got, ref, row), tag
    assert np.abs(got['out'][row]).max() <= CF and not got['out'][row][:HOP].any() and got['out'][row][HOP:].any()


# -------------------------------------------------------------------------------------------------------- parity against the reference
def test_parity_with_the_reference_on_one_stream():
    """(B, hops) = (1, 12), the speech at +6 dB, 5 hops per call"""
    key = ('speech', 6.0, 0, 12)
    check_parity('(1, 12) +6 dB', feed(_lim(1), [K.named(key)], 5), 0, K.ref_run(key))


def test_parity_with_the_reference_on_three_shifted_streams():
    """(B, hops) = (3, 40), 7 hops per call, the streams shifted by 5000 samples against each other and at -3, +6 and +12 dB: a
    transparent, a moderately and a heavily limited stream share the launch"""
    keys = [('speech', over, 5000 * i, 40) for i, over in enumerate(K.OVERS)]
    got = feed(_lim(3), [K.named(k) for k in keys], 7)
    for i, key in enumerate(keys):
        check_parity('(3, 40) stream %d at %+g dB' % (i, key[1]), got, i, K.ref_run(key))
    assert np.all(got['gain'][0, HOP:] == 1.0) and got['gain'][1, HOP:].min() < 0.9 and got['gain'][2, HOP:].min() < 0.5


@pytest.mark.parametrize('kw', [{'lookahead': 1}, {'lookahead': 192}, {'true_peak': False}, {'drive': 4.0}], ids=lambda kw: '%s_%s' % tuple(kw.items())[0])
def test_parity_with_the_reference_at_other_settings(kw):
    """(2, 12) at LA = 1 and LA = 192: the speech at +12 dB and a tone that starts 6 dB over; (1, 12) without the taps and with drive 4"""
    keys = [('speech', 0.0 if 'drive' in kw else 12.0, 0, 12)] + ([('tone', 5333.0)] if 'lookahead' in kw else [])
    pkw = dict(kw)
    if 'drive' in pkw:
        pkw['drive_db'] = 20.0 * np.log10(pkw.pop('drive'))
    lim = _lim(len(keys), **pkw)
    rkw = dict(kw, drive=lim.drive) if 'drive' in kw else kw              # (the factor the object computed from its dB)
    got = feed(lim, [K.named(k) for k in keys], 5)
    for i, key in enumerate(keys):
        check_parity('%s %s' % (kw, key), got, i, K.ref_run(key, **rkw))
        assert got['gain'][i, HOP:].min() < 0.6


# ------------------------------------------------------------------------------------------------------------ the properties on the device
def test_the_ceiling_holds_on_noise_four_times_over():
    """(4, 16), uniform noise of amplitude 4 c: max |out| <= cf, and gain times the driven input never exceeds cf as float32 - the
    clamp does not act"""
    rs = np.random.RandomState(26)
    x = (4.0 * CEILING * rs.uniform(-1.0, 1.0, (4, 16 * HOP))).astype(np.float32)
    got = feed(_lim(4), list(x), 16)
    y = (got['gain'][:, HOP:] * x[:, :-HOP].astype(np.float64)).astype(np.float32)
    print('noise at 4 c: max |out| / cf = %.9f, max |(float)(g s)| / cf = %.9f, smallest gain %.4f' % (np.abs(got['out']).max() / CF, np.abs(y).max() / CF, got['gain'][:, HOP:].min()))
    assert np.abs(got['out']).max() <= CF and np.abs(y).max() <= CF and np.array_equal(bits(y), bits(got['out'][:, HOP:]))
    assert got['gain'][:, HOP:].min() < 0.3 and got['peak'][:, 1:].min() > 3.0 * CEILING


def test_below_the_ceiling_the_output_is_the_input_one_hop_late():
    x = K.speech(-3.0, hops=24)
    got = feed(_lim(1), [x], 24)
    assert np.array_equal(bits(got['out'][0, HOP:]), bits(x[:-HOP])) and np.all(got['gain'][0, HOP:] == 1.0) and not got['gain'][0, :HOP].any()
    assert 0 < got['peak'][0, 1:].max() < CEILING


# ---------------------------------------------------------------------------------------------------------------- bitwise invariances
def streams(n, hops=24):
    return [K.speech(12.0, shift=5000 * i, hops=hops) for i in range(n)]


def test_hop_grouping_and_batch_do_not_change_a_slot():
    xs = streams(5)
    runs = [feed(_lim(1), [xs[3]], group) for group in (1, 7, 24)]
    for r in runs[1:]:
        assert same(r, runs[0])
    assert all(np.isfinite(runs[0][k]).all() for k in runs[0]) and runs[0]['gain'][0, HOP:].min() < 0.5
    five = feed(_lim(5), xs, 5)                                            # the same stream in slot 3 of B = 5, the other slots busy
    assert same(cut(five, slice(3, 4)), runs[0])
    assert not np.array_equal(five['out'][2], five['out'][3])


def _record(lim, slot):
    from nele_gan_amd import _lib
    rec = int(_lib.lib.nele_lim_stream_record_bytes(lim.lookahead))
    header = lim.nbytes - lim.S * rec
    assert header == 256
    return lim.state[header + slot * rec:header + (slot + 1) * rec].clone()


def test_inactive_slots_are_neither_read_nor_written():
    B, n0, n1 = 3, 10, 6
    xs = streams(B)
    lim = _lim(B)
    feed(lim, [x[:n0 * HOP] for x in xs], 4)
    before = _record(lim, 1)
    assert before.any()
    X = np.stack([x[n0 * HOP:(n0 + n1) * HOP] for x in xs])               # a call that skips slot 1: NaN rows there, sentinel outputs
    X[1] = np.nan
    out = (torch.full((B, n1 * HOP), SENTINEL, device='cuda'), torch.full((B, n1 * HOP), SENTINEL, dtype=torch.float64, device='cuda'),
           torch.full((B, n1), SENTINEL, dtype=torch.float64, device='cuda'))
    got = lim.process(torch.from_numpy(X), active=[True, False, True], want=WANT, out=out)
    assert all(g is o for g, o in zip(got, out))
    for t in got:
        assert (t[1] == SENTINEL).all() and not (t[0] == SENTINEL).any() and not (t[2] == SENTINEL).any() and torch.isfinite(t).all()
    assert torch.equal(_record(lim, 1), before)
    assert list(lim.hops) == [n0 + n1, n0, n0 + n1]
    later = feed(lim, [xs[1][n0 * HOP:]], 5, slots=[1])                    # slot 1 goes on where it was
    alone = feed(_lim(1), [xs[1]], 24)
    assert same(later, cut(alone, hops=slice(n0, None)))


def test_reset_restarts_one_slot_and_leaves_the_others():
    B, n0 = 3, 10
    xs = streams(B)
    fresh = feed(_lim(1), [xs[1][:(24 - n0) * HOP]], 14)
    assert not fresh['out'][0, :HOP].any() and not fresh['gain'][0, :HOP].any() and fresh['peak'][0, 0] == 0     # a slot's first hop

    def run(with_reset):
        lim = _lim(B)
        feed(lim, [x[:n0 * HOP] for x in xs], 4)
        if with_reset:
            lim.reset([1])
            assert not _record(lim, 1).any() and _record(lim, 0).any()
            assert list(lim.hops) == [n0, 0, n0]
        x2 = [x[n0 * HOP:] for x in xs]
        if with_reset:
            x2[1] = xs[1][:(24 - n0) * HOP]
        return feed(lim, x2, 7)

    r, r_ = run(True), run(False)
    assert same(cut(r, slice(1, 2)), fresh)
    for s in (0, 2):
        assert same(cut(r, slice(s, s + 1)), cut(r_, slice(s, s + 1)))
    assert not np.array_equal(r['out'][1], r_['out'][1])


def test_a_state_laid_out_for_another_lookahead_is_not_touched():
    """the kernel compares the geometry header: given LA = 40 on a state that init laid out for LA = 80 (large enough), it writes nothing"""
    import ctypes
    from nele_gan_amd import _lib
    lim = _lim(2)
    feed(lim, streams(2, hops=4), 4)
    before = lim.state.clone()
    x = torch.from_numpy(np.stack(streams(2, hops=1))).cuda()
    out = torch.full((2, HOP), SENTINEL, device='cuda')
    taps = (ctypes.c_double * 36)(*lim.taps.reshape(-1))
    _lib.call('nele_lim_hop', _lib.ptr(lim.state), ctypes.c_longlong(lim.nbytes), 2, _lib.ptr(x), None, 1, lim.ceiling, lim.drive, 40, lim.rel,
              taps, _lib.ptr(out), None, None, _lib.stream())
    assert torch.equal(lim.state, before) and (out == SENTINEL).all()


def test_settings_reach_the_kernel():
    x = K.speech(12.0, hops=12)
    low = _lim(1, ceiling_db=-6.0)
    a, b, c = feed(_lim(1), [x], 12), feed(_lim(1, release=0.01), [x], 12), feed(low, [x], 12)
    assert not np.array_equal(a['gain'], b['gain']) and np.array_equal(a['peak'], b['peak'])
    assert 0.99 * low.ceiling < np.abs(c['out']).max() <= floor32(low.ceiling) < 0.51
    with pytest.raises(ValueError, match='want'):
        _lim(1).process(torch.zeros(1, HOP), want=('gains',))
    o, pk = _lim(1).process(torch.from_numpy(x[None, :2 * HOP].copy()), want='peak')
    assert o.shape == (1, 2 * HOP) and pk.shape == (1, 2) and pk.dtype == torch.float64


# --------------------------------------------------------------------------------------------------------- behind the enhancer
def _rt(streams):
    from nele_gan_amd.realtime import RealtimeEnhancer
    from nele_gan_amd.siiopt import SiiOptRule
    return RealtimeEnhancer(rule=SiiOptRule(), streams=streams)


def _drc(streams):
    from nele_gan_amd.drc import StreamCompressor
    return StreamCompressor(streams)


def _compressed(streams):
    from nele_gan_amd.drc import CompressedEnhancer
    return CompressedEnhancer(_rt(streams), _drc(streams))


def _two_streams(hops, scale=25.0):
    """two scenarios of tests/siiopt_cases.py, loud enough (rms 0.75) for the limiter to act behind the enhancer"""
    import siiopt_cases as SK
    a, b = SK.scenario('ssn', -5.0), SK.scenario('pink', -5.0)
    cl = scale * np.stack([a['speech'][:hops * HOP], b['speech'][3000:3000 + hops * HOP]])
    ns = scale * np.stack([a['noise'][:hops * HOP], b['noise'][3000:3000 + hops * HOP]])
    return cl.astype(np.float32), ns.astype(np.float32)


@pytest.mark.parametrize('inner', ['rule', 'compressed'])
def test_limited_enhancer_is_the_objects_chained_by_hand(inner):
    from nele_gan_amd.limiter import LimitedEnhancer
    hops, group, k = 16, 5, 100
    cl, ns = _two_streams(hops + 1)
    make = _rt if inner == 'rule' else _compressed
    chain, hand_in, hand_lim = LimitedEnhancer(make(2), _lim(2)), make(2), _lim(2)
    assert chain.S == 2 and chain.lag_hops == (2 if inner == 'rule' else 3)
    limited = False
    for a in range(0, hops * HOP, group * HOP):
        b = min(hops * HOP, a + group * HOP)
        c, v = torch.from_numpy(cl[:, a:b].copy()), torch.from_numpy(ns[:, a:b].copy())
        got, mid = chain.process(c, v), hand_in.process(c, v)
        assert torch.equal(got, hand_lim.process(mid)), a
        limited = limited or mid.abs().max().item() > CEILING
        assert got.abs().max().item() <= CF
    assert limited and got.abs().max().item() > 0
    # finish slot 1 alone, with a tail of k samples: the inner object's last hops and one zero hop through the limiter
    tc, tn = np.zeros((1, HOP), np.float32), np.zeros((1, HOP), np.float32)
    tc[0, :k], tn[0, :k] = cl[1, hops * HOP:hops * HOP + k], ns[1, hops * HOP:hops * HOP + k]
    end = chain.finish([1], tc, tn, [k])
    last = hand_in.finish([1], tc, tn, [k])
    n_in = 1 if inner == 'rule' else 2
    assert last.shape == (1, n_in * HOP) and end.shape == (1, (n_in + 1) * HOP)                 # one hop more than the inner finish
    full = torch.zeros(2, (n_in + 1) * HOP, device='cuda')
    full[1, :n_in * HOP] = last[0]
    hand = hand_lim.process(full, active=[False, True])
    assert torch.equal(end[0], hand[1]) and end[0, HOP:].abs().max().item() > 0
    assert list(chain.lim.hops) == [hops, hops + n_in + 1]
    chain.reset([1])
    assert list(chain.lim.hops) == [hops, 0] and not _record(chain.lim, 1).any() and _record(chain.lim, 0).any()


def test_inside_the_echo_loop_the_canceller_sees_the_limited_signal():
    """B = 2, P = 2, 8 hops"""
    from nele_gan_amd.aec import EchoCanceller, EchoCancellingEnhancer
    from nele_gan_amd.limiter import LimitedEnhancer
    NH, CALLS = 2, 4
    cl, ns = _two_streams(NH * CALLS)
    loop = EchoCancellingEnhancer(LimitedEnhancer(_rt(2), _lim(2)), EchoCanceller(2, partitions=2))
    hand_aec, hand_rt, hand_lim = EchoCanceller(2, partitions=2), _rt(2), _lim(2)
    played = torch.zeros(2, NH * HOP, device='cuda')
    acted = False
    for c in range(CALLS):
        cols = slice(c * NH * HOP, (c + 1) * NH * HOP)
        clean = torch.from_numpy(cl[:, cols].copy())
        mic = torch.from_numpy((ns[:, cols] + 0.5 * played.cpu().numpy()).astype(np.float32))       # the noise and an echo of what was played
        out = loop.process(clean, mic)
        rule_out = hand_rt.process(clean, hand_aec.process(mic, played))
        limited = hand_lim.process(rule_out)
        assert torch.equal(out, limited) and torch.equal(loop.played, limited), c
        acted = acted or rule_out.abs().max().item() > CEILING
        played = limited
    assert acted and torch.isfinite(out).all() and out.abs().max().item() > 0 and out.abs().max().item() <= CF


def test_the_wrapper_with_the_band_knows_the_limited_chains_lag():
    """48 kHz, B = 1: adapt(EchoCancellingEnhancer(LimitedEnhancer(CompressedEnhancer(..), lim), aec), 48000, highband=True).latency is
    the HighBandUp's lag for 3 hops, 960 + 2 x 768, and a unit impulse in ``clean`` leaves at that latency with the band (the carried
    impulse) and without it (the low band through the real chain)."""
    from nele_gan_amd.aec import EchoCanceller, EchoCancellingEnhancer
    from nele_gan_amd.highband import highband_plan
    from nele_gan_amd.limiter import LimitedEnhancer
    from nele_gan_amd.streamrate import RateAdaptedEnhancer, adapt, adapt_fullband
    rate, hops, hop, t0 = 48000, 8, 768, 768 + 300
    rs = np.random.RandomState(48)
    clean = (1e-3 * rs.randn(1, hops * hop)).astype(np.float32)
    clean[0, t0] = 1.0
    second = (0.05 * rs.randn(1, hops * hop)).astype(np.float32)

    def inner():
        return EchoCancellingEnhancer(LimitedEnhancer(_compressed(1), _lim(1)), EchoCanceller(1, partitions=2))

    def through(w):
        return torch.cat([w.process(torch.from_numpy(clean[:, k * hop:(k + 2) * hop]), torch.from_numpy(second[:, k * hop:(k + 2) * hop]))
                          for k in range(0, hops, 2)], dim=1).cpu().numpy()
    wrap, plain = adapt(inner(), rate, highband=True), RateAdaptedEnhancer(inner(), rate)
    assert wrap.up.lag_hops == 3 and wrap.latency == wrap.up.lag == highband_plan(rate, 3)['lag'] == 960 + 2 * 768
    assert adapt_fullband(inner(), rate).latency == wrap.latency
    got, low_only = through(wrap), through(plain)
    peak, peak_low = int(np.abs(got[0]).argmax()), int(np.abs(low_only[0]).argmax())
    print('impulse at %d, peak of |out| at %d, of the low band alone at %d, latency %d' % (t0, peak, peak_low, wrap.latency))
    assert (peak - t0, peak_low - t0) == (wrap.latency, wrap.latency)


# ----------------------------------------------------------------------------------------------------------------------- command line
def test_command_line(tmp_path, capsys):
    from nele_gan_amd import dataio
    from nele_gan_amd import limiter as M
    L = 30 * HOP + 100
    in_path, out_path = str(tmp_path / 'in.wav'), str(tmp_path / 'out.wav')
    dataio.write_wav_pcm16(in_path, K.speech(-2.0, hops=31)[:L])                     # fits PCM_16; 12 dB of drive put it 10 dB over the ceiling
    assert M.main(['--in', in_path, '--out', out_path, '--drive-db', '12']) == 0
    said = capsys.readouterr().out
    x, _ = dataio.read_wav(in_path)
    d = np.zeros((1, 32 * HOP), np.float32)
    d[0, :L] = x
    want = _lim(1, drive_db=12.0).process(torch.from_numpy(d))[0, HOP:HOP + L].cpu().numpy()
    assert 'limited' in said and ' 0 clipped samples' in said and int(np.sum(np.abs(want) * np.float32(32767.0) > 32767.5)) == 0
    assert np.abs(want).max() > 0.99 * CF                                              # it was limited: at drive 12 dB the input peaks 10 dB over
    out, sr = dataio.read_wav(out_path)
    assert sr == 16000 and out.shape == (L,)
    assert np.array_equal(out, dataio.pcm16_quantise(want).astype(np.float32) / np.float32(32768.0)) and out[L - 100:].any()
    with pytest.raises(SystemExit):
        M.main(['--in', in_path, '--out', out_path, '--lookahead-ms', '13'])
    assert 'lookahead' in capsys.readouterr().err
