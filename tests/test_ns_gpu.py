"""GPU: the noise suppressor (nele_gan_amd/ns.py, csrc/ns.hip) against tests/ns_ref.py - the float64 numpy restatement of DESIGN.md
section 21 - its streaming contract (grouping, batch, slots, skipped calls, reset: bitwise, for the output and the three optional
outputs), the figures of section 21's table, DuplexEnhancer around the closed loop and both command lines.

Bounds (tests/ns_cases.py): |G_gpu - G_ref|, |p_gpu - p_ref|, lambda_D relative and |out_gpu - out_ref| over the peak are each held to
8 x the all-flipped sensitivity that tests/test_ns_cpu.py measures on the same inputs (every float32 power moved one ulp up or down at
random): a GPU run flips few of those roundings - its transform differs from numpy's by some 1e-16 of a frame's peak - where that
experiment flips all; the factor covers the spread between seeds and the exp / log / E1 implementations.  No hop, bin or stream is left
out.
Measured on an MI355X: at (B, hops) = (1, 40) gains 1.4e-15 (bound 2.5e-6), presence 2.2e-16 (4.2e-6), noise_psd 4.4e-16 (3.7e-6), output
3.9e-18 of the peak (5.0e-7); at (3, 264) gains 1.3e-15 / 1.7e-15 / 1.8e-15 (4.2e-6 / 5.2e-6 / 3.0e-6), presence 2.2e-16, noise_psd 5.6e-16 /
6.7e-16 / 6.7e-16, output 1.1e-17 / 2.5e-18 / 9.5e-18 of the peak.  Every float32 sample bit-equal to the reference's except in a stream's
first hop (the zero history: rounding noise near 1e-18 on both sides).  First scenario's figures: 10.215 dB, -1.263 dB and 0.1690 for
the reference and for the GPU."""

import numpy as np
import pytest

import aec_cases as C
import ns_cases as K
from ns_ref import HOP, NBINS

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

SENTINEL = -7.25
WANT = ('gains', 'noise_psd', 'presence')
_DRIVEN = {}


def _ns(B, **kw):
    from nele_gan_amd.ns import NoiseSuppressor
    return NoiseSuppressor(B, **kw)


def feed(ns, xs, group, slots=None):
    """all hops of the given streams through ``ns`` (in ``slots``, default 0 ..), ``group`` hops per call at most
    -> dict: out [n, L] float32; gains, noise_psd, presence [n, L / 256, 257] float64, on the host"""
    slots = list(range(len(xs))) if slots is None else slots
    L = len(xs[0])
    parts = {k: [] for k in ('out',) + WANT}
    for a in range(0, L, group * HOP):
        b = min(L, a + group * HOP)
        X = np.full((ns.S, b - a), np.nan, np.float32)
        act = np.zeros(ns.S, bool)
        for i, s in enumerate(slots):
            X[s], act[s] = xs[i][a:b], True
        got = ns.process(torch.from_numpy(X), active=None if act.all() else act, want=WANT)
        for k, t in zip(('out',) + WANT, got):
            parts[k].append(t[slots].cpu().numpy())
    return {k: np.concatenate(v, axis=1) for k, v in parts.items()}


def cut(d, rows=slice(None), hops=slice(None)):
    """the rows (streams) and hops of every output of a feed()"""
    samples = slice(None if hops.start is None else hops.start * HOP, None if hops.stop is None else hops.stop * HOP)
    return dict({k: d[k][rows, hops] for k in WANT}, out=d['out'][rows, samples])


def same(a, b):
    """the output and the three optional outputs, bit for bit"""
    return all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]) for k in ('out',) + WANT)


def check_parity(tag, got, ref, key):
    """one stream against the reference's run, every hop and bin, under GPU_FACTOR x the recorded sensitivity of these inputs"""
    peak = float(np.abs(ref['out']).max())
    dev = {'gains': float(np.abs(got['gains'] - ref['gains']).max()), 'presence': float(np.abs(got['presence'] - ref['presence']).max()),
           'noise_psd': float(np.abs(got['noise_psd'] / ref['noise_psd'] - 1.0).max()),
           'out': float(np.abs(got['out'].astype(np.float64) - ref['out'].astype(np.float64)).max()) / peak}
    bound = {k: K.GPU_FACTOR * v for k, v in K.SENS[key].items()}
    print('%s: %s; %d of %d samples differ' % (tag, ', '.join('%s %.3g (bound %.3g)' % (k, dev[k], bound[k]) for k in dev),
                                              int((got['out'] != ref['out']).sum()), ref['out'].size))
    assert got['out'].dtype == np.float32 and got['gains'].shape == ref['gains'].shape == (len(ref['out']) // HOP, NBINS)
    for k in dev:
        assert np.isfinite(got[k]).all() and dev[k] <= bound[k], (tag, k, dev[k], bound[k])


def streams(n, hops=40):
    """n different inputs of ``hops`` hops: the pink 10 dB scenario, circularly shifted"""
    x = K.scenario('pink', 10.0)['x']
    return [np.roll(x, -5000 * i)[:hops * HOP].copy() for i in range(n)]


# -------------------------------------------------------------------------------------------------------- parity against the reference
def test_parity_with_the_reference_on_one_stream():
    """(B, hops) = (1, 40), 11 hops per call: frame 15 and the first minima store at frame 30"""
    key = ('pink', 10.0, 40)
    got = feed(_ns(1), [K.scenario(*key)['x']], 11)
    check_parity('(1, 40)', {k: v[0] for k, v in got.items()}, K.ref_run(*key), key)


def driven():
    """the three scenarios of section 21's table as one batch of three, 264 hops, 13 hops per call: run once, shared"""
    if not _DRIVEN:
        _DRIVEN.update(feed(_ns(3), [K.scenario(kind, snr)['x'] for kind, snr in K.SCENARIOS], 13))
    return _DRIVEN


def test_parity_with_the_reference_on_the_three_scenarios():
    """(B, hops) = (3, 264), 13 hops per call: the minima ring wraps at frame 135"""
    got = driven()
    for i, (kind, snr) in enumerate(K.SCENARIOS):
        check_parity('(3, 264) stream %d, %s %g dB' % (i, kind, snr), {k: v[i] for k, v in got.items()}, K.ref_run(kind, snr), (kind, snr, 264))


def test_the_figures_of_the_first_scenario_are_the_references():
    kind, snr = K.SCENARIOS[0]
    s, ref, got = K.scenario(kind, snr), K.ref_run(kind, snr), driven()
    fr = K.figures(s['speech'], s['noise'], ref['out'], ref['gains'])
    fg = K.figures(s['speech'], s['noise'], got['out'][0], got['gains'][0])
    print('%s %g dB, reference / GPU: noise attenuated %.3f / %.3f dB, speech level %.3f / %.3f dB, error ratio after %.4f / %.4f'
          % (kind, snr, fr[0], fg[0], fr[1], fg[1], fr[3], fg[3]))
    assert abs(fg[0] - fr[0]) <= K.GPU_FIGURES_WITHIN_DB and abs(fg[1] - fr[1]) <= K.GPU_FIGURES_WITHIN_DB
    assert abs(10.0 * np.log10(fg[3] / fr[3])) <= K.GPU_FIGURES_WITHIN_DB
    assert fg[0] >= K.MIN_NOISE_ATTENUATION_DB and fg[1] >= K.MIN_SPEECH_LEVEL_CHANGE_DB and fg[3] <= K.MAX_ERROR_RATIO_OF_INPUTS * fg[2]
    assert fg[4] <= K.MAX_SPLIT


# ---------------------------------------------------------------------------------------------------------------- bitwise invariances
def test_hop_grouping_and_batch_do_not_change_a_slot():
    xs = streams(5)
    runs = [feed(_ns(1), [xs[3]], group) for group in (1, 7, 40)]
    for r in runs[1:]:
        assert same(r, runs[0])
    assert all(np.isfinite(runs[0][k]).all() for k in runs[0]) and runs[0]['gains'].min() < 0.2 and runs[0]['presence'].max() > 0.9
    # the same stream in slot 3 of B = 5, the other slots busy with their own
    five = feed(_ns(5), xs, 5)
    assert same(cut(five, slice(3, 4)), runs[0])
    assert not np.array_equal(five['out'][2], five['out'][3])


def _record(ns, slot):
    from nele_gan_amd import _lib
    rec = int(_lib.lib.nele_ns_stream_record_bytes())
    header = ns.nbytes - ns.S * rec
    return ns.state[header + slot * rec:header + (slot + 1) * rec].clone()


def test_inactive_slots_are_neither_read_nor_written():
    B, n0, n1 = 3, 18, 6
    xs = streams(B)
    ns = _ns(B)
    feed(ns, [x[:n0 * HOP] for x in xs], 4)
    before = _record(ns, 1)
    assert before.any()
    # a call that skips slot 1: NaN input rows there, sentinel-filled outputs
    X = np.stack([x[n0 * HOP:(n0 + n1) * HOP] for x in xs])
    X[1] = np.nan
    out = (torch.full((B, n1 * HOP), SENTINEL, device='cuda'),) + tuple(
        torch.full((B, n1, NBINS), SENTINEL, dtype=torch.float64, device='cuda') for _ in WANT)
    got = ns.process(torch.from_numpy(X), active=[True, False, True], want=WANT, out=out)
    assert all(g is o for g, o in zip(got, out))
    for t in got:
        assert (t[1] == SENTINEL).all() and not (t[0] == SENTINEL).any() and not (t[2] == SENTINEL).any() and torch.isfinite(t).all()
    assert torch.equal(_record(ns, 1), before)
    assert list(ns.hops) == [n0 + n1, n0, n0 + n1]
    # slot 1 goes on where it was: equal to a run that never saw the skipped call
    later = feed(ns, [xs[1][n0 * HOP:]], 5, slots=[1])
    alone = feed(_ns(1), [xs[1]], 40)
    assert same(later, cut(alone, hops=slice(n0, None)))


def test_reset_restarts_one_slot_and_leaves_the_others():
    B, n0 = 3, 18
    xs = streams(B)
    fresh = feed(_ns(1), [xs[1][:(40 - n0) * HOP]], 22)

    def run(with_reset):
        ns = _ns(B)
        feed(ns, [x[:n0 * HOP] for x in xs], 4)
        if with_reset:
            ns.reset([1])
            assert not _record(ns, 1).any() and _record(ns, 0).any()
            assert list(ns.hops) == [n0, 0, n0]
        x2 = [x[n0 * HOP:] for x in xs]
        if with_reset:
            x2[1] = xs[1][:(40 - n0) * HOP]
        return feed(ns, x2, 7)

    r = run(True)
    assert same(cut(r, slice(1, 2)), fresh)
    r_ = run(False)
    for s in (0, 2):
        assert same(cut(r, slice(s, s + 1)), cut(r_, slice(s, s + 1)))
    assert not np.array_equal(r['out'][1], r_['out'][1])


def test_settings_reach_the_kernel():
    x = streams(1, hops=20)[0]
    a, b = feed(_ns(1), [x], 20), feed(_ns(1, gmin=0.25), [x], 20)
    assert np.abs(a['gains'][0, :15] - 0.1).max() <= 1e-15 and np.abs(b['gains'][0, :15] - 0.25).max() <= 1e-15
    assert not a['presence'][0, :15].any() and a['presence'][0, 15:].any()
    one = feed(_ns(1, gmin=1.0), [x], 20)
    assert np.array_equal(one['out'][0, HOP:15 * HOP], x[:14 * HOP])              # gmin = 1: the input, one hop late
    with pytest.raises(ValueError, match='want'):
        _ns(1).process(torch.zeros(1, HOP), want=('gain',))
    o, p = _ns(1).process(torch.from_numpy(x[None, :HOP].copy()), want='presence')
    assert o.shape == (1, HOP) and p.shape == (1, 1, NBINS) and p.dtype == torch.float64


# --------------------------------------------------------------------------------------------------------------------- both directions
def test_duplex_enhancer_around_the_closed_loop():
    """The set-up of tests/test_aec_gpu.py's closed loop (B = 2, P = 8, 4 hops per call, its generator, room and noise scaling), 16
    calls.  First the existing loop alone, recorded before any wrapper exists.  Then DuplexEnhancer in a room of its own: its `out` is
    the recording bit for bit (so the microphone signals are the same too), its uplink is NoiseSuppressor.process on the residual of
    a canceller chained by hand, bit for bit; reset restarts both objects."""
    from nele_gan_amd.aec import EchoCancellingEnhancer, EchoCanceller
    from nele_gan_amd.ns import DuplexEnhancer
    from nele_gan_amd.realtime import RealtimeEnhancer
    from test_aec_gpu import _generator, _Room, scen
    B, P, NH, CALLS = 2, 8, 4, 16
    W = NH * HOP
    G = _generator()
    ss = [scen(P, i) for i in range(B)]
    clean = np.stack([s['played'] for s in ss])
    noise = np.stack([s['noise'] for s in ss])
    hs = [s['h'] for s in ss]

    def loop():
        return EchoCancellingEnhancer(RealtimeEnhancer(G=G, streams=B, precision='f32'), EchoCanceller(B, partitions=P))

    plain, room, recorded, mics = loop(), _Room(hs, noise, W), [], []
    for c in range(CALLS):
        m, _ = room.mic()
        out = plain.process(torch.from_numpy(clean[:, c * W:(c + 1) * W].copy()), torch.from_numpy(m))
        assert isinstance(out, torch.Tensor)
        recorded.append(out.clone())
        mics.append(m)
        room.play(out.cpu().numpy())

    duplex = DuplexEnhancer(loop(), _ns(B))
    hand_aec, hand_ns = EchoCanceller(B, partitions=P), _ns(B)
    room = _Room(hs, noise, W)
    played = torch.zeros((B, W), device='cuda')
    for c in range(CALLS):
        m, _ = room.mic()
        assert np.array_equal(m, mics[c]), c
        out, uplink = duplex.process(torch.from_numpy(clean[:, c * W:(c + 1) * W].copy()), torch.from_numpy(m))
        assert torch.equal(out, recorded[c]), c
        residual = hand_aec.process(torch.from_numpy(m), played)
        assert torch.equal(uplink, hand_ns.process(residual)), c
        assert torch.isfinite(uplink).all() and uplink.shape == out.shape
        played = out
        room.play(out.cpu().numpy())
    assert uplink.abs().max() > 0
    duplex.reset([1])
    assert list(duplex.ns.hops) == [CALLS * NH, 0] and list(duplex.loop.aec.hops) == [CALLS * NH, 0]
    assert not _record(duplex.ns, 1).any() and _record(duplex.ns, 0).any()


# ----------------------------------------------------------------------------------------------------------------------- command lines
def _pcm(t):
    from nele_gan_amd import dataio
    return dataio.pcm16_quantise(t[0].cpu().numpy()).astype(np.float32) / np.float32(32768.0)


def test_command_line_of_the_suppressor(tmp_path, capsys):
    from nele_gan_amd import dataio
    from nele_gan_amd import ns as N
    L = 30 * HOP + 100
    in_path, out_path = str(tmp_path / 'in.wav'), str(tmp_path / 'out.wav')
    dataio.write_wav_pcm16(in_path, K.scenario('pink', 10.0)['x'][:L])
    assert N.main(['--in', in_path, '--out', out_path, '--gmin', '0.2']) == 0
    assert 'one hop' in capsys.readouterr().out
    x, _ = dataio.read_wav(in_path)
    d = np.zeros((1, 31 * HOP), np.float32)
    d[0, :L] = x
    out, sr = dataio.read_wav(out_path)
    assert sr == 16000 and out.shape == (L,)
    assert np.array_equal(out, _pcm(_ns(1, gmin=0.2).process(torch.from_numpy(d)))[:L]) and out[16 * HOP:].any()
    for bad in ('0', '1.5'):
        with pytest.raises(SystemExit):
            N.main(['--in', in_path, '--out', out_path, '--gmin', bad])
        assert '--gmin' in capsys.readouterr().err


def test_command_line_of_the_canceller_writes_the_uplink(tmp_path, capsys):
    from nele_gan_amd import aec as A
    from nele_gan_amd import dataio
    P = 3
    s = C.scenario(1, 700, 0.08, 10.0, hops=40)
    L = 30 * HOP + 100
    paths = {n: str(tmp_path / (n + '.wav')) for n in ('mic', 'played', 'out', 'out2', 'up')}
    dataio.write_wav_pcm16(paths['mic'], s['mic'][:L])
    dataio.write_wav_pcm16(paths['played'], s['played'][:L])
    base = ['--mic', paths['mic'], '--played', paths['played'], '--partitions', str(P)]
    assert A.main(base + ['--out', paths['out']]) == 0
    assert 'uplink' not in capsys.readouterr().out
    assert A.main(base + ['--out', paths['out2'], '--uplink', paths['up'], '--uplink-gmin', '0.2']) == 0
    assert 'noise suppressed' in capsys.readouterr().out
    assert open(paths['out'], 'rb').read() == open(paths['out2'], 'rb').read()    # --out does not notice the flag
    mic, _ = dataio.read_wav(paths['mic'])
    pl, _ = dataio.read_wav(paths['played'])
    d, x = np.zeros((1, 31 * HOP), np.float32), np.zeros((1, 31 * HOP), np.float32)
    d[0, :L], x[0, :L] = mic, pl
    res = A.EchoCanceller(1, partitions=P).process(torch.from_numpy(d), torch.from_numpy(x))
    out, _ = dataio.read_wav(paths['out'])
    assert np.array_equal(out, _pcm(res)[:L])              # without the flag: the canceller's residual, as before
    res[0, L:] = 0.0                                       # the file's residual is cut at L and padded again
    up, sr = dataio.read_wav(paths['up'])
    assert sr == 16000 and up.shape == (L,)
    assert np.array_equal(up, _pcm(_ns(1, gmin=0.2).process(res))[:L]) and up[16 * HOP:].any()
    for bad in (['--uplink-gmin', '0.2'], ['--uplink', paths['up'], '--uplink-gmin', '0']):
        with pytest.raises(SystemExit):
            A.main(base + ['--out', paths['out2']] + bad)
        assert '--uplink-gmin' in capsys.readouterr().err
