"""GPU: the residual-echo suppressor (nele_gan_amd/res.py, csrc/res.hip) against tests/res_ref.py - the float64 numpy restatement of
DESIGN.md section 17 - its streaming contract (grouping, batch, slots, reset: bitwise), the closed loop around RealtimeEnhancer and the
command line.

Bounds.  Gains: |G_gpu - G_ref| <= 1e-8.  The floor and eps bound the conditioning of step 3: G = sqrt(u) with u >= gmin^2 = 1e-2, so
dG = du / (2 G) <= 5 du, and u = 1 - beta R / (S_ee + eps) moves by a few 1e-15 relative to its terms when the transforms differ by
1e-15 of a frame's peak.  Output: |out_gpu - float32 out_ref| <= 2^-21 max |out_ref| - one float32 rounding flip (2^-24 of a value, at
most 2^-23 of the peak after the sum of two windowed halves) plus the gain's share.
Measured on an MI355X (largest values): gains 6.9e-13 and output 8.8e-17 of the peak at (B, hops) = (1, 40); gains 4.9e-13 and output
1.6e-16 at (3, 264) behind the real canceller; gains 8.9e-13 at beta = 4, gmin = 0.25.  Every float32 sample bit-equal to the reference's
except in a stream's first hop (the zero history: rounding noise near 1e-17 on both sides).  echo = 0: every sample equal to the input
one hop earlier, the first hop 1.1e-17 of the peak.  Suppression on section 17's first scenario: 4.595 dB and -1.269 dB for the reference
and for the GPU.  Closed loop: see test_closed_loop_around_the_realtime_enhancer."""
import numpy as np
import pytest

import aec_cases as C
from res_cases import SCENARIOS, figures, ref_run
from res_ref import HOP, NBINS, ResRef

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

SENTINEL = -7.25
G_BOUND, OUT_BOUND = 1e-8, 2.0 ** -21
_DRIVEN = {}


def _res(B, **kw):
    from nele_gan_amd.res import ResidualEchoSuppressor
    return ResidualEchoSuppressor(B, **kw)


def _aec(B, P):
    from nele_gan_amd.aec import EchoCanceller
    return EchoCanceller(B, partitions=P)


def feed(res, es, ys, group, slots=None):
    """all hops of the given streams through ``res`` (in ``slots``, default 0 ..), ``group`` hops per call at most
    -> (out [n, L] float32, gains [n, L / 256, 257] float64) on the host"""
    slots = list(range(len(es))) if slots is None else slots
    L = len(es[0])
    outs, gains = [], []
    for a in range(0, L, group * HOP):
        b = min(L, a + group * HOP)
        E = np.full((res.S, b - a), np.nan, np.float32)
        Y = np.full((res.S, b - a), np.nan, np.float32)
        act = np.zeros(res.S, bool)
        for i, s in enumerate(slots):
            E[s], Y[s], act[s] = es[i][a:b], ys[i][a:b], True
        o, g = res.process(torch.from_numpy(E), torch.from_numpy(Y), active=None if act.all() else act, want_gains=True)
        outs.append(o[slots].cpu().numpy())
        gains.append(g[slots].cpu().numpy())
    return np.concatenate(outs, axis=1), np.concatenate(gains, axis=1)


def check_parity(tag, out, G, out_ref, G_ref):
    dg = float(np.abs(G - G_ref).max())
    do = float(np.abs(out.astype(np.float64) - out_ref.astype(np.float64)).max() / np.abs(out_ref).max())
    print('%s: gains %.3g (bound 1e-8), output %.3g of the peak (bound 2^-21 = %.3g), %d of %d samples differ'
          % (tag, dg, do, OUT_BOUND, int((out != out_ref).sum()), out.size))
    assert G.shape == G_ref.shape and out.dtype == np.float32
    assert dg <= G_BOUND, (tag, dg)
    assert do <= OUT_BOUND, (tag, do)


def first(hops=264):
    """the first scenario of section 17's table: (e, y) float32 as the reference canceller leaves them, the reference's run"""
    run = ref_run(*SCENARIOS[0])
    return run['e'][:hops * HOP], run['y'][:hops * HOP], run


def streams(n, hops=40):
    """n different (e, y) pairs of ``hops`` hops: the first scenario's, circularly shifted"""
    e, y, _ = first()
    return [np.roll(e, -5000 * i)[:hops * HOP].copy() for i in range(n)], [np.roll(y, -5000 * i)[:hops * HOP].copy() for i in range(n)]


# -------------------------------------------------------------------------------------------------------- parity against the reference
def test_parity_with_the_reference_on_one_stream():
    """(B, hops) = (1, 40), 11 hops per call: the inputs are the reference canceller's"""
    e, y, run = first(40)
    out, G = feed(_res(1), [e], [y], 11)
    check_parity('B 1, 40 hops', out[0], G[0], run['out'][:40 * HOP], run['G'][:40])


def driven():
    """(B, hops) = (3, 264): EchoCanceller at P = 3 on tests/test_aec_gpu.py's three scenarios gives residual and echo on the GPU; the
    reference suppressor runs on those.  Computed once, shared, never changed -> (residual, echo [3, L] float32, [(out, G)] per slot)"""
    if not _DRIVEN:
        from test_aec_gpu import scen
        ss = [scen(3, i) for i in range(3)]
        r, y = _aec(3, 3).process(torch.from_numpy(np.stack([s['mic'] for s in ss])), torch.from_numpy(np.stack([s['played'] for s in ss])),
                                  want_echo=True)
        _DRIVEN['e'], _DRIVEN['y'] = r.cpu().numpy(), y.cpu().numpy()
        _DRIVEN['ref'] = [ResRef().run(_DRIVEN['e'][i], _DRIVEN['y'][i]) for i in range(3)]
    return _DRIVEN['e'], _DRIVEN['y'], _DRIVEN['ref']


def test_parity_with_the_reference_behind_the_real_canceller():
    e, y, ref = driven()
    out, G = feed(_res(3), list(e), list(y), 13)
    for i in range(3):
        check_parity('B 3, 264 hops, slot %d' % i, out[i], G[i], *ref[i])
        assert G[i].min() < 0.5 and G[i].max() > 0.99          # the gain is at work: the comparison is not 1 = 1


# ---------------------------------------------------------------------------------------------------------------- bitwise invariances
def test_hop_grouping_and_batch_do_not_change_a_slot():
    es, ys = streams(5)
    runs = [feed(_res(1), [es[3]], [ys[3]], group) for group in (1, 7, 40)]
    for r in runs[1:]:
        assert np.array_equal(r[0], runs[0][0]) and np.array_equal(r[1], runs[0][1])
    assert np.isfinite(runs[0][0]).all() and runs[0][1].min() < 0.9
    # the same stream in slot 3 of B = 5, the other slots busy with their own
    out, G = feed(_res(5), es, ys, 5)
    assert np.array_equal(out[3], runs[0][0][0]) and np.array_equal(G[3], runs[0][1][0])
    assert not np.array_equal(out[2], out[3])


def _record(res, slot):
    from nele_gan_amd import _lib
    rec = int(_lib.lib.nele_res_stream_record_bytes())
    header = res.nbytes - res.S * rec
    return res.state[header + slot * rec:header + (slot + 1) * rec].clone()


def test_inactive_slots_are_neither_read_nor_written():
    B, n0, n1 = 3, 10, 6
    es, ys = streams(B)
    res = _res(B)
    feed(res, [e[:n0 * HOP] for e in es], [y[:n0 * HOP] for y in ys], 4)
    before = _record(res, 1)
    assert before.any()
    # a call that skips slot 1: NaN inputs there, sentinel-filled outputs
    E = np.stack([e[n0 * HOP:(n0 + n1) * HOP] for e in es])
    Y = np.stack([y[n0 * HOP:(n0 + n1) * HOP] for y in ys])
    E[1], Y[1] = np.nan, np.nan
    out = (torch.full((B, n1 * HOP), SENTINEL, device='cuda'), torch.full((B, n1, NBINS), SENTINEL, dtype=torch.float64, device='cuda'))
    o, g = res.process(torch.from_numpy(E), torch.from_numpy(Y), active=[True, False, True], want_gains=True, out=out)
    assert o is out[0] and g is out[1]
    assert (o[1] == SENTINEL).all() and (g[1] == SENTINEL).all()
    for s in (0, 2):
        assert not (o[s] == SENTINEL).any() and not (g[s] == SENTINEL).any()
    assert torch.equal(_record(res, 1), before)
    assert list(res.hops) == [n0 + n1, n0, n0 + n1]
    # slot 1 goes on where it was: equal to a run that never saw the skipped call
    o1, g1 = feed(res, [es[1][n0 * HOP:]], [ys[1][n0 * HOP:]], 5, slots=[1])
    oa, ga = feed(_res(1), [es[1]], [ys[1]], 40)
    assert np.array_equal(o1[0], oa[0][n0 * HOP:]) and np.array_equal(g1[0], ga[0][n0:])


def test_reset_restarts_one_slot_and_leaves_the_others():
    B, n0 = 3, 12
    es, ys = streams(B)
    of, gf = feed(_res(1), [es[1][:(40 - n0) * HOP]], [ys[1][:(40 - n0) * HOP]], 28)

    def run(with_reset):
        res = _res(B)
        feed(res, [e[:n0 * HOP] for e in es], [y[:n0 * HOP] for y in ys], 4)
        if with_reset:
            res.reset([1])
            assert not _record(res, 1).any() and _record(res, 0).any()
            assert list(res.hops) == [n0, 0, n0]
        e2, y2 = [e[n0 * HOP:] for e in es], [y[n0 * HOP:] for y in ys]
        if with_reset:
            e2[1], y2[1] = es[1][:(40 - n0) * HOP], ys[1][:(40 - n0) * HOP]
        return feed(res, e2, y2, 7)

    o, g = run(True)
    assert np.array_equal(o[1], of[0]) and np.array_equal(g[1], gf[0])
    o_, g_ = run(False)
    for s in (0, 2):
        assert np.array_equal(o[s], o_[s]) and np.array_equal(g[s], g_[s])
    assert not np.array_equal(o[1], o_[1])


# ------------------------------------------------------------------------------------------------------------------- what it computes
def test_without_an_echo_estimate_the_output_is_the_input_one_hop_late():
    """echo = 0: G is exactly 1 and the output of hop h is hop h - 1 of the input within 1e-14 max |e| (the CPU test's bound)"""
    e = C.scenario(1, 700, 0.08, 10.0, hops=40)['mic']
    out, G = feed(_res(1), [e], [np.zeros_like(e)], 9)
    assert np.array_equal(G[0], np.ones((40, NBINS)))
    worst = float(np.abs(out[0][HOP:].astype(np.float64) - e[:-HOP]).max() / np.abs(e).max())
    first_hop = float(np.abs(out[0][:HOP]).max() / np.abs(e).max())
    print('echo = 0: largest |out - input one hop earlier| = %.3g max |e|, first hop %.3g (bound 1e-14)' % (worst, first_hop))
    assert worst <= 1e-14 and first_hop <= 1e-14


def test_it_suppresses():
    """the first scenario of section 17's table: the GPU's suppression of the residual echo and its change of the noise level are
    within 0.02 dB of the reference's (4.60 dB and -1.27 dB)"""
    e, y, run = first()
    out, G = feed(_res(1), [e], [y], 264)
    sup_ref, lvl_ref, _ = figures(run['e'], run['noise'], run['out'], run['G'])
    sup, lvl, split = figures(run['e'], run['noise'], out[0], G[0])
    print('residual echo suppressed: reference %.3f dB, GPU %.3f dB; noise level: reference %+.3f dB, GPU %+.3f dB; split %.3g'
          % (sup_ref, sup, lvl_ref, lvl, split))
    assert sup_ref >= 3.0 and abs(lvl_ref) <= 1.5
    assert abs(sup - sup_ref) <= 0.02 and abs(lvl - lvl_ref) <= 0.02
    assert split <= 3.0 * 2.0 ** -24


def test_settings_reach_the_kernel():
    """beta = 0 is a pass-through with G = 1; gmin is the floor the gains reach; a larger beta takes out more"""
    e, y, _ = first(40)
    _, G0 = feed(_res(1, beta=0.0), [e], [y], 40)
    assert np.array_equal(G0[0], np.ones((40, NBINS)))
    _, G1 = feed(_res(1, beta=4.0, gmin=0.25), [e], [y], 40)
    _, G2 = feed(_res(1, beta=1.0, gmin=0.25), [e], [y], 40)
    assert G1.min() == 0.25 and G2.min() >= 0.25 and (G1 <= G2).all() and (G1 < G2).any()
    r = ResRef(beta=4.0, gmin=0.25).run(e, y)
    check_parity('beta 4, gmin 0.25', feed(_res(1, beta=4.0, gmin=0.25), [e], [y], 40)[0][0], G1[0], *r)


# ------------------------------------------------------------------------------------------------------------------------ closed loop
def test_closed_loop_around_the_realtime_enhancer():
    """The set-up of tests/test_aec_gpu.py's closed loop (B = 2, P = 8, 4 hops per call, 256 hops and a tail of 100 samples, its
    generator, room and noise scaling), the canceller wrapped in SuppressedEchoCanceller.  The loop object against the three stages
    chained by hand - with the canceller's own residual in the first hop, as SuppressedEchoCanceller hands it on: a RealtimeEnhancer
    whose noise input starts on the suppressor's silent first hop puts out NaN from frame 15 on - bit-identical, finish included.
    Then, over the second half, beside a loop without the suppressor:
    sum (noise input - true noise)^2 / sum noise^2 (with the suppressor both one hop late), and the mean relative error of the dbg_noise
    band powers (band ** 6) against a run on the true noise (with the suppressor against the true run's previous frame).
    Measured on an MI355X, second half: sum (noise input - noise)^2 / sum noise^2 = 0.206 with the suppressor, 0.495 with the canceller
    alone; mean relative error of the dbg_noise band powers against the true-noise run: 0.255 with the suppressor, 1.7 without.
    Asserted: the first ratio is lower with the suppressor than without."""
    from nele_gan_amd.aec import EchoCancellingEnhancer
    from nele_gan_amd.realtime import RealtimeDebug, RealtimeEnhancer
    from nele_gan_amd.res import SuppressedEchoCanceller
    from test_aec_gpu import _generator, _Room, scen
    B, P, NH, CALLS, TAIL = 2, 8, 4, 64, 100
    W, L = NH * HOP, NH * HOP * CALLS
    G = _generator()
    ss = [scen(P, i) for i in range(B)]
    clean = np.stack([s['played'] for s in ss])
    noise = np.stack([s['noise'] for s in ss])
    hs = [s['h'] for s in ss]
    T = L // HOP + 2

    def rt():
        return RealtimeEnhancer(G=G, streams=B, precision='f32')

    # ---- the loop object and the chain by hand, in lockstep on the same microphone signal
    loop, dbg = EchoCancellingEnhancer(rt(), SuppressedEchoCanceller(_aec(B, P), _res(B))), RealtimeDebug(B, T)
    hand_rt, hand_aec, hand_res = rt(), _aec(B, P), _res(B)
    room = _Room(hs, noise, W)
    played = torch.zeros((B, W), device='cuda')
    fed = np.zeros((B, L))                                 # what the enhancer was given as noise
    for c in range(CALLS):
        m, _ = room.mic()
        cl = torch.from_numpy(clean[:, c * W:(c + 1) * W].copy())
        out = loop.process(cl, torch.from_numpy(m), debug=dbg)
        e, y = hand_aec.process(torch.from_numpy(m), played, want_echo=True)
        sup = hand_res.process(e, y)
        if c == 0:
            sup[:, :HOP] = e[:, :HOP]
        played = hand_rt.process(cl, sup)
        assert torch.isfinite(played).all(), c
        assert torch.equal(out, played), c
        fed[:, c * W:(c + 1) * W] = sup.cpu().numpy()
        room.play(out.cpu().numpy())
    m, _ = room.mic(TAIL)
    ct, mt = np.zeros((B, HOP), np.float32), np.zeros((B, HOP), np.float32)
    ct[:, :TAIL], mt[:, :TAIL] = clean[:, L:L + TAIL], m
    last = loop.finish([0, 1], ct, mt, [TAIL, TAIL], debug=dbg)
    e, y = hand_aec.process(torch.from_numpy(mt), played[:, :HOP].contiguous(), want_echo=True)
    assert torch.equal(last, hand_rt.finish([0, 1], ct, hand_res.process(e, y).cpu(), [TAIL, TAIL]))
    assert list(loop.rt.emitted) == [L, L]

    # ---- the canceller alone, its own loop
    plain, plain_dbg = EchoCancellingEnhancer(rt(), _aec(B, P)), RealtimeDebug(B, T)
    plain_aec = _aec(B, P)                                 # in lockstep, to read the residual the loop's enhancer is given
    room = _Room(hs, noise, W)
    residual = np.zeros((B, L))
    pl = torch.zeros((B, W), device='cuda')
    for c in range(CALLS):
        m, _ = room.mic()
        residual[:, c * W:(c + 1) * W] = plain_aec.process(torch.from_numpy(m), pl).cpu().numpy()
        pl = plain.process(torch.from_numpy(clean[:, c * W:(c + 1) * W].copy()), torch.from_numpy(m), debug=plain_dbg)
        room.play(pl.cpu().numpy())

    # ---- the true noise
    true_rt, true_dbg = rt(), RealtimeDebug(B, T)
    true_rt.process(torch.from_numpy(clean[:, :L].copy()), torch.from_numpy(noise[:, :L].astype(np.float32)), debug=true_dbg)
    torch.cuda.synchronize()

    half, late = slice(L // 2, L), slice(L // 2 - HOP, L - HOP)
    with_res = float(np.sum((fed[:, half] - noise[:, late]) ** 2) / np.sum(noise[:, late] ** 2))
    without = float(np.sum((residual[:, half] - noise[:, half]) ** 2) / np.sum(noise[:, half] ** 2))
    f, fl = slice(L // 2 // HOP, L // HOP), slice(L // 2 // HOP - 1, L // HOP - 1)
    tn, tl = true_dbg.noise[:, f].double() ** 6, true_dbg.noise[:, fl].double() ** 6
    err_res = float((((dbg.noise[:, f].double() ** 6) - tl).abs() / tl).mean())
    err_plain = float((((plain_dbg.noise[:, f].double() ** 6) - tn).abs() / tn).mean())
    print('closed loop, second half: sum (noise input - noise)^2 / sum noise^2 = %.4g with the suppressor, %.4g with the canceller alone'
          % (with_res, without))
    print('closed loop, second half: mean relative error of dbg_noise ** 6 against the true-noise run: %.4g with the suppressor, %.4g without'
          % (err_res, err_plain))
    assert with_res < without


# ----------------------------------------------------------------------------------------------------------------------- command line
def test_command_line(tmp_path, capsys):
    from nele_gan_amd import aec as A
    from nele_gan_amd import dataio
    from nele_gan_amd.res import SuppressedEchoCanceller
    P = 3
    s = C.scenario(1, 700, 0.08, 10.0, hops=40)
    L = 30 * HOP + 100
    mic_path, pl_path, out_path, sup_path = (str(tmp_path / n) for n in ('mic.wav', 'played.wav', 'out.wav', 'sup.wav'))
    dataio.write_wav_pcm16(mic_path, s['mic'][:L])
    dataio.write_wav_pcm16(pl_path, s['played'][:L])
    base = ['--mic', mic_path, '--played', pl_path, '--partitions', str(P)]
    assert A.main(base + ['--out', out_path]) == 0
    assert 'suppress' not in capsys.readouterr().out
    assert A.main(base + ['--out', sup_path, '--suppress', '--res-beta', '1.5', '--res-gmin', '0.2']) == 0
    assert 'one hop' in capsys.readouterr().out
    mic, _ = dataio.read_wav(mic_path)
    pl, _ = dataio.read_wav(pl_path)
    n = L // HOP * HOP
    d, x = torch.from_numpy(mic[None, :n].copy()), torch.from_numpy(pl[None, :n].copy())

    def pcm(t):
        return dataio.pcm16_quantise(t[0].cpu().numpy()).astype(np.float32) / np.float32(32768.0)

    out, sr = dataio.read_wav(out_path)                    # without the flag: the canceller's residual, as before
    assert sr == 16000 and out.shape == (L,)
    assert np.array_equal(out[:n], pcm(_aec(1, P).process(d, x)))
    sup, sr = dataio.read_wav(sup_path)
    assert sr == 16000 and sup.shape == (L,)
    want = SuppressedEchoCanceller(_aec(1, P), _res(1, beta=1.5, gmin=0.2)).process(d, x)
    assert np.array_equal(sup[:n], pcm(want)) and not np.array_equal(sup[HOP:n], out[:n - HOP])
    assert np.array_equal(sup[:HOP], out[:HOP])            # the first hop: the canceller's own residual
    for bad in (['--res-beta', '-1'], ['--res-gmin', '0'], ['--res-gmin', '1.5']):
        with pytest.raises(SystemExit):
            A.main(base + ['--out', sup_path, '--suppress'] + bad)
        assert '--res-beta' in capsys.readouterr().err
