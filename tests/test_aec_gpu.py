"""GPU: the echo canceller (nele_gan_amd/aec.py, csrc/aec.hip) against tests/aec_ref.py - the float64 numpy restatement of DESIGN.md
section 14 - its streaming contract (grouping, batch, slots, reset: bitwise), and the closed loop around RealtimeEnhancer.

Bounds.  Echo path: max |h_gpu - h_ref| <= 1e-10 max |h_ref| (float64 rounding stays near 1e-14: the step is smooth, no thresholds; a
wrong ring index, conjugate, constraint or partition costs more than 1e-2).  float32 outputs: |residual_gpu - float32(e_ref)| <=
2^-22 max |e_ref|, likewise echo (one float32 rounding flip).
Measured on an MI355X (largest ratios; every float32 residual and echo sample came out bit-equal to float32 of the reference's, ratio 0):
echo path 3.4e-16 at (B, P) = (1, 1); 5.8e-16 at (3, 3), the unpaired partition; 1.07e-15 at (2, 32), 40 hops; 6.5e-16 at (5, 8) with
ragged active masks over 33 ring wraps; 9.4e-16 after adaptation was frozen and resumed.  echo against np.convolve(played,
echo_path()): 5.6e-8 of the peak (bound 1e-6).  Echo reduction over the second half at P = 3, 700 taps, T60 0.08 s, ENR 10 dB:
reference 14.20 dB, GPU 14.20 dB (this file's path seed; the prototype's draw gave 15.6 dB; bound >= 10 dB, within 0.01 dB).
Closed loop: see test_closed_loop_around_the_realtime_enhancer."""
import os

import numpy as np
import pytest

import aec_cases as C
from aec_ref import HOP, AecRef

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from weights_recipe import seeded_state_arrays  # noqa: E402

SENTINEL = -7.25
SHAPES = {1: (200, 0.03), 2: (450, 0.05), 3: (700, 0.08), 8: (1900, 0.15), 32: (8000, 0.4)}      # P -> (taps, T60) of the scenario's path
_SCEN, _REF = {}, {}


def scen(P, slot, hops=264, enr_db=10.0):
    """the scenario of slot ``slot`` of a batch at P partitions: its own path seed and circular shift"""
    key = (P, slot, hops, enr_db)
    if key not in _SCEN:
        taps, t60 = SHAPES[P]
        _SCEN[key] = C.scenario(seed=100 * P + slot, taps=taps, t60=t60, enr_db=enr_db, shift=4001 * slot, hops=hops)
    return _SCEN[key]


def ref_run(P, slot, hops=264):
    """(e, y, h) of the reference on scen(P, slot, hops): computed once, shared, never changed"""
    key = (P, slot, hops)
    if key not in _REF:
        s = scen(P, slot, hops)
        r = AecRef(P)
        e, y = r.run(s['mic'], s['played'])
        _REF[key] = (e, y, r.echo_path())
    return _REF[key]


def _aec(B, P, **kw):
    from nele_gan_amd.aec import EchoCanceller
    return EchoCanceller(B, partitions=P, **kw)


def feed(aec, mics, playeds, group, slots=None, adapt=None):
    """all hops of the given streams through ``aec`` (in ``slots``, default 0 ..), ``group`` hops per call at most
    -> (residual [n, L], echo [n, L]) on the host"""
    slots = list(range(len(mics))) if slots is None else slots
    L = len(mics[0])
    res, echo = [], []
    for a in range(0, L, group * HOP):
        b = min(L, a + group * HOP)
        D = np.zeros((aec.S, b - a), np.float32)
        X = np.zeros((aec.S, b - a), np.float32)
        act = np.zeros(aec.S, bool)
        for i, s in enumerate(slots):
            D[s], X[s], act[s] = mics[i][a:b], playeds[i][a:b], True
        r, y = aec.process(torch.from_numpy(D), torch.from_numpy(X), active=None if act.all() else act, adapt=adapt, want_echo=True)
        res.append(r[slots].cpu().numpy())
        echo.append(y[slots].cpu().numpy())
    return np.concatenate(res, axis=1), np.concatenate(echo, axis=1)


def check_parity(tag, res, echo, h, e_ref, y_ref, h_ref):
    rh = float(np.abs(h - h_ref).max() / np.abs(h_ref).max())
    re_ = float(np.abs(res.astype(np.float64) - e_ref.astype(np.float32)).max() / np.abs(e_ref).max())
    ry = float(np.abs(echo.astype(np.float64) - y_ref.astype(np.float32)).max() / np.abs(y_ref).max())
    print('%s: echo path %.3g (bound 1e-10), residual %.3g, echo %.3g (bound 2^-22 = %.3g)' % (tag, rh, re_, ry, 2.0 ** -22))
    assert rh <= 1e-10, (tag, rh)
    assert re_ <= 2.0 ** -22, (tag, re_)
    assert ry <= 2.0 ** -22, (tag, ry)
    return rh, re_, ry


# -------------------------------------------------------------------------------------------------------- parity against the reference
@pytest.mark.parametrize('B,P,hops', [(1, 1, 264), (3, 3, 264), (2, 32, 40)])
def test_parity_with_the_reference(B, P, hops):
    """every slot of the batch against the reference on its own scenario; (3, 3): the unpaired partition"""
    ss = [scen(P, i, hops) for i in range(B)]
    aec = _aec(B, P)
    res, echo = feed(aec, [s['mic'] for s in ss], [s['played'] for s in ss], 11)
    h = aec.echo_path().cpu().numpy()
    for i in range(B):
        check_parity('B %d P %d slot %d' % (B, P, i), res[i], echo[i], h[i], *ref_run(P, i, hops))


def test_parity_with_ragged_active_masks_and_ring_wrap():
    """B = 5, P = 8, 264 hops (the ring wraps 33 times): each call brings 8 hops to a random subset of the slots, the others are
    inactive and their input rows hold NaN - a slot that is read while inactive poisons its state"""
    B, P, G = 5, 8, 8
    ss = [scen(P, i) for i in range(B)]
    aec = _aec(B, P)
    rng = np.random.RandomState(7)
    pos = np.zeros(B, int)
    res = [[] for _ in range(B)]
    echo = [[] for _ in range(B)]
    while (pos < 264).any():
        act = (rng.rand(B) < 0.6) & (pos < 264)
        if not act.any():
            continue
        D = np.full((B, G * HOP), np.nan, np.float32)
        X = np.full((B, G * HOP), np.nan, np.float32)
        for i in np.nonzero(act)[0]:
            D[i], X[i] = ss[i]['mic'][pos[i] * HOP:(pos[i] + G) * HOP], ss[i]['played'][pos[i] * HOP:(pos[i] + G) * HOP]
        r, y = aec.process(torch.from_numpy(D), torch.from_numpy(X), active=act, want_echo=True)
        r, y = r.cpu().numpy(), y.cpu().numpy()
        for i in np.nonzero(act)[0]:
            res[i].append(r[i])
            echo[i].append(y[i])
            pos[i] += G
    h = aec.echo_path().cpu().numpy()
    assert list(aec.hops) == [264] * B
    for i in range(B):
        check_parity('ragged slot %d' % i, np.concatenate(res[i]), np.concatenate(echo[i]), h[i], *ref_run(P, i))


def test_echo_is_the_convolution_with_the_exported_path():
    """echo of a hop = np.convolve(played history, echo_path() read before that call) on that hop, to 1e-6 of its peak (float32)"""
    P = 3
    s = scen(P, 0)
    aec = _aec(1, P)
    worst = peak = 0.0
    for m in range(40):
        h = aec.echo_path()[0].cpu().numpy()
        _, y = aec.process(torch.from_numpy(s['mic'][None, m * HOP:(m + 1) * HOP].copy()), torch.from_numpy(s['played'][None, m * HOP:(m + 1) * HOP].copy()),
                           want_echo=True)
        want = np.convolve(s['played'][:(m + 1) * HOP].astype(np.float64), h)[m * HOP:(m + 1) * HOP]
        y = y[0].cpu().numpy().astype(np.float64)
        peak = max(peak, float(np.abs(want).max()))
        worst = max(worst, float(np.abs(y - want).max() / max(np.abs(want).max(), 1e-30)))
    assert peak > 0.0 and np.abs(aec.echo_path()[0].cpu().numpy()).max() > 1e-2          # the filter has moved: the identity is not 0 = 0
    print('echo against np.convolve(played, echo_path()): %.3g of the peak' % worst)
    assert worst <= 1e-6


# ---------------------------------------------------------------------------------------------------------------- bitwise invariances
@pytest.mark.parametrize('P', [3, 8])
def test_hop_grouping_and_batch_do_not_change_a_slot(P):
    s = scen(P, 3)
    runs = []
    for group in (1, 7, 264):
        aec = _aec(1, P)
        res, echo = feed(aec, [s['mic']], [s['played']], group)
        runs.append((res[0], echo[0], aec.echo_path()[0].cpu().numpy()))
    for r in runs[1:]:
        for a, b in zip(r, runs[0]):
            assert np.array_equal(a, b)
    # the same stream in slot 3 of B = 5, the other slots busy with their own
    ss = [scen(P, i) for i in range(5)]
    aec = _aec(5, P)
    res, echo = feed(aec, [x['mic'] for x in ss], [x['played'] for x in ss], 5)
    assert np.array_equal(res[3], runs[0][0]) and np.array_equal(echo[3], runs[0][1])
    assert np.array_equal(aec.echo_path([3])[0].cpu().numpy(), runs[0][2])


def _record(aec, slot):
    from nele_gan_amd import _lib
    rec = int(_lib.lib.nele_aec_stream_record_bytes(aec.P))
    header = aec.nbytes - aec.S * rec
    return aec.state[header + slot * rec:header + (slot + 1) * rec].clone()


def test_inactive_slots_are_neither_read_nor_written():
    B, P, n0, n1 = 3, 2, 10, 6
    ss = [scen(P, i, hops=40) for i in range(B)]
    mics, pls = [s['mic'] for s in ss], [s['played'] for s in ss]
    aec = _aec(B, P)
    feed(aec, [m[:n0 * HOP] for m in mics], [p[:n0 * HOP] for p in pls], 4)
    before = _record(aec, 1)
    # a call that skips slot 1: NaN inputs there, sentinel-filled outputs
    D = np.stack([m[n0 * HOP:(n0 + n1) * HOP] for m in mics])
    X = np.stack([p[n0 * HOP:(n0 + n1) * HOP] for p in pls])
    D[1], X[1] = np.nan, np.nan
    out = (torch.full((B, n1 * HOP), SENTINEL, device='cuda'), torch.full((B, n1 * HOP), SENTINEL, device='cuda'))
    aec.process(torch.from_numpy(D), torch.from_numpy(X), active=[True, False, True], want_echo=True, out=out)
    assert (out[0][1] == SENTINEL).all() and (out[1][1] == SENTINEL).all()
    assert not (out[0][0] == SENTINEL).any() and not (out[0][2] == SENTINEL).any()
    assert torch.equal(_record(aec, 1), before)
    # slot 1 goes on where it was: equal to a run that never saw the skipped call
    r1, y1 = feed(aec, [mics[1][n0 * HOP:]], [pls[1][n0 * HOP:]], 5, slots=[1])
    alone = _aec(1, P)
    ra, ya = feed(alone, [mics[1]], [pls[1]], 40)
    assert np.array_equal(r1[0], ra[0][n0 * HOP:]) and np.array_equal(y1[0], ya[0][n0 * HOP:])
    assert np.array_equal(aec.echo_path([1]).cpu().numpy(), alone.echo_path().cpu().numpy())


def test_frozen_adaptation_keeps_the_path_and_resumes_like_the_reference():
    P, a, b, c = 3, 20, 10, 10                               # hops adapting, frozen, adapting again
    s = scen(P, 1, hops=40)
    mic, pl = s['mic'], s['played']
    aec = _aec(1, P)
    ref = AecRef(P)
    r0, y0 = feed(aec, [mic[:a * HOP]], [pl[:a * HOP]], 6)
    e0, _ = ref.run(mic[:a * HOP], pl[:a * HOP])
    h_before = aec.echo_path()[0].cpu().numpy()
    r1, y1 = feed(aec, [mic[a * HOP:(a + b) * HOP]], [pl[a * HOP:(a + b) * HOP]], 3, adapt=[False])
    h_frozen = aec.echo_path()[0].cpu().numpy()
    assert np.array_equal(h_before, h_frozen) and np.abs(h_frozen).max() > 1e-2
    e1, yr1 = ref.run(mic[a * HOP:(a + b) * HOP], pl[a * HOP:(a + b) * HOP], adapt=False)
    assert np.abs(r1[0].astype(np.float64) - e1.astype(np.float32)).max() <= 2.0 ** -22 * np.abs(e1).max()
    # the residual is still d - y, y the frozen filter's output
    want = np.convolve(pl[:(a + b) * HOP].astype(np.float64), h_frozen)[a * HOP:(a + b) * HOP]
    assert np.abs(r1[0] - (mic[a * HOP:(a + b) * HOP] - want)).max() <= 1e-6 * np.abs(mic).max()
    # S_e kept running while frozen: resuming matches a reference that did the same
    r2, y2 = feed(aec, [mic[(a + b) * HOP:]], [pl[(a + b) * HOP:]], 4)
    e2, yr2 = ref.run(mic[(a + b) * HOP:], pl[(a + b) * HOP:])
    check_parity('resumed', r2[0], y2[0], aec.echo_path()[0].cpu().numpy(), e2, yr2, ref.echo_path())
    assert not np.array_equal(aec.echo_path()[0].cpu().numpy(), h_frozen)


def test_reset_restarts_one_slot_and_leaves_the_others():
    B, P, n0 = 3, 3, 12
    ss = [scen(P, i, hops=40) for i in range(B)]
    mics, pls = [s['mic'] for s in ss], [s['played'] for s in ss]
    fresh = _aec(1, P)
    rf, yf = feed(fresh, [mics[1][:(40 - n0) * HOP]], [pls[1][:(40 - n0) * HOP]], 28)

    def run(with_reset):
        aec = _aec(B, P)
        feed(aec, [m[:n0 * HOP] for m in mics], [p[:n0 * HOP] for p in pls], 4)
        if with_reset:
            aec.reset([1])
            assert not aec.echo_path([1]).any() and aec.echo_path([0]).any()
        m2 = [m[n0 * HOP:] for m in mics]
        p2 = [p[n0 * HOP:] for p in pls]
        if with_reset:
            m2[1], p2[1] = mics[1][:(40 - n0) * HOP], pls[1][:(40 - n0) * HOP]
        r, y = feed(aec, m2, p2, 7)
        return r, y, aec.echo_path().cpu().numpy()

    r, y, h = run(True)
    assert np.array_equal(r[1], rf[0]) and np.array_equal(y[1], yf[0]) and np.array_equal(h[1], fresh.echo_path()[0].cpu().numpy())
    r_, y_, h_ = run(False)
    for s in (0, 2):
        assert np.array_equal(r[s], r_[s]) and np.array_equal(y[s], y_[s]) and np.array_equal(h[s], h_[s])


def test_silence_played_passes_the_microphone_through():
    P = 3
    s = scen(P, 2, hops=40)
    aec = _aec(1, P)
    res, echo = feed(aec, [s['mic']], [np.zeros_like(s['played'])], 9)
    assert np.array_equal(res[0], s['mic'])
    assert not echo.any() and not aec.echo_path().any()


def test_it_cancels():
    """P = 3, 700 taps, T60 0.08 s, ENR 10 dB: the echo reduction over the second half of the signal.  The prototype of section 14
    measured 15.6 dB for the reference; the kernel must be within 0.01 dB of the reference."""
    P = 3
    s = scen(P, 0)
    e_ref, y_ref, _ = ref_run(P, 0)
    aec = _aec(1, P)
    res, echo = feed(aec, [s['mic']], [s['played']], 264)
    red_ref, red_gpu = C.reduction_db(s['echo'], y_ref), C.reduction_db(s['echo'], echo[0].astype(np.float64))
    print('echo reduction over the second half: reference %.2f dB, GPU %.2f dB' % (red_ref, red_gpu))
    assert red_ref >= 10.0
    assert abs(red_gpu - red_ref) <= 0.01


# ------------------------------------------------------------------------------------------------------------------------ closed loop
def _generator():
    from nele_gan_amd import model
    G = model.Generator_Conv1D_cLN()
    sd = G.state_dict()
    arrs = seeded_state_arrays([(k, tuple(v.shape)) for k, v in sd.items()], 101)
    G.load_state_dict({k: torch.from_numpy(v) for k, v in arrs.items()})
    return G.cuda()


class _Room:
    """the listener's room on the host: the loudspeaker plays what the last call returned, the microphone hears noise plus its echo"""

    def __init__(self, hs, noise, width):
        self.hs, self.noise, self.W = hs, noise, width
        self.ls = np.zeros((len(hs), noise.shape[1] + 2 * width))       # the loudspeaker signal: out of call c at columns [(c + 1) W, (c + 2) W)
        self.c = 0

    def mic(self, width=None):
        a, b = self.c * self.W, self.c * self.W + (self.W if width is None else width)
        echo = np.zeros((len(self.hs), b - a))
        for i, h in enumerate(self.hs):
            lo = max(0, a - len(h) + 1)
            echo[i] = np.convolve(self.ls[i, lo:b], h)[a - lo:b - lo]
        return (self.noise[:, a:b] + echo).astype(np.float32), echo

    def play(self, out):
        self.ls[:, (self.c + 1) * self.W:(self.c + 2) * self.W] = out
        self.c += 1


def test_closed_loop_around_the_realtime_enhancer():
    """B = 2, P = 8, 4 hops per call, 256 hops and a tail of 100 samples; the noise is scaled to 10 dB below the echo the clean far end
    itself would leave (the enhancer keeps the clean level).  EchoCancellingEnhancer against the chain by hand (bitwise), then against
    the raw microphone fed in as noise: sum (residual - noise)^2 / sum noise^2 over the second half, and the mean relative error of the
    dbg_noise band powers (band ** 6) against a run on the true noise.
    Measured on an MI355X, second half: sum (residual - noise)^2 / sum noise^2 = 0.495 with the canceller, 13.9 with the raw microphone
    (the echo 11.4 dB above the noise there, 3.1 dB below it after cancellation); mean relative error of the dbg_noise band powers
    against the true-noise run: 1.7 with the canceller, 27.7 without.  The loop object and the chain by hand: bit-identical, finish
    included."""
    from nele_gan_amd.aec import EchoCancellingEnhancer
    from nele_gan_amd.realtime import RealtimeDebug, RealtimeEnhancer
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

    def tails(room):
        m, echo = room.mic(TAIL)
        ct, mt = np.zeros((B, HOP), np.float32), np.zeros((B, HOP), np.float32)
        ct[:, :TAIL], mt[:, :TAIL] = clean[:, L:L + TAIL], m
        return ct, mt

    # ---- the loop object and the chain by hand, in lockstep on the same microphone signal
    loop, dbg = EchoCancellingEnhancer(rt(), _aec(B, P)), RealtimeDebug(B, T)
    hand_rt, hand_aec = rt(), _aec(B, P)
    room = _Room(hs, noise, W)
    played = torch.zeros((B, W), device='cuda')
    residual = np.zeros((B, L))
    for c in range(CALLS):
        m, _ = room.mic()
        cl = torch.from_numpy(clean[:, c * W:(c + 1) * W].copy())
        out = loop.process(cl, torch.from_numpy(m), debug=dbg)
        res = hand_aec.process(torch.from_numpy(m), played)
        played = hand_rt.process(cl, res)
        assert torch.equal(out, played), c
        residual[:, c * W:(c + 1) * W] = res.cpu().numpy()
        room.play(out.cpu().numpy())
    ct, mt = tails(room)
    last = loop.finish([0, 1], ct, mt, [TAIL, TAIL], debug=dbg)
    res = hand_aec.process(torch.from_numpy(mt), played[:, :HOP].contiguous())
    assert torch.equal(last, hand_rt.finish([0, 1], ct, res.cpu(), [TAIL, TAIL]))
    assert list(loop.rt.emitted) == [L, L]

    # ---- the raw microphone as `noise`, its own loop
    raw_rt, raw_dbg = rt(), RealtimeDebug(B, T)
    room = _Room(hs, noise, W)
    raw_mic = np.zeros((B, L))
    for c in range(CALLS):
        m, _ = room.mic()
        raw_mic[:, c * W:(c + 1) * W] = m
        out = raw_rt.process(torch.from_numpy(clean[:, c * W:(c + 1) * W].copy()), torch.from_numpy(m), debug=raw_dbg)
        room.play(out.cpu().numpy())

    # ---- the true noise
    true_rt, true_dbg = rt(), RealtimeDebug(B, T)
    true_rt.process(torch.from_numpy(clean[:, :L].copy()), torch.from_numpy(noise[:, :L].astype(np.float32)), debug=true_dbg)
    torch.cuda.synchronize()

    half = slice(L // 2, L)
    den = np.sum(noise[:, half] ** 2)
    with_aec = float(np.sum((residual[:, half] - noise[:, half]) ** 2) / den)
    without = float(np.sum((raw_mic[:, half] - noise[:, half]) ** 2) / den)
    f = slice(L // 2 // HOP, L // HOP)
    tn = true_dbg.noise[:, f].double() ** 6
    err_aec = float((((dbg.noise[:, f].double() ** 6) - tn).abs() / tn).mean())
    err_raw = float((((raw_dbg.noise[:, f].double() ** 6) - tn).abs() / tn).mean())
    print('closed loop, second half: sum (residual - noise)^2 / sum noise^2 = %.4g with the canceller, %.4g with the raw microphone' % (with_aec, without))
    print('closed loop, second half: mean relative error of dbg_noise ** 6 against the true-noise run: %.4g with the canceller, %.4g without'
          % (err_aec, err_raw))
    assert with_aec < without


# ----------------------------------------------------------------------------------------------------------------------- command line
def test_command_line(tmp_path, capsys):
    from nele_gan_amd import aec as A
    from nele_gan_amd import dataio
    P = 3
    s = scen(P, 0, hops=40)
    L = 30 * HOP + 100
    mic_path, pl_path, out_path, h_path = (str(tmp_path / n) for n in ('mic.wav', 'played.wav', 'out.wav', 'h.npy'))
    dataio.write_wav_pcm16(mic_path, s['mic'][:L])
    dataio.write_wav_pcm16(pl_path, s['played'][:L])
    assert A.main(['--mic', mic_path, '--played', pl_path, '--out', out_path, '--partitions', str(P), '--echo-path', h_path]) == 0
    out, sr = dataio.read_wav(out_path)
    assert sr == 16000 and out.shape == (L,)
    mic, _ = dataio.read_wav(mic_path)
    pl, _ = dataio.read_wav(pl_path)
    n = L // HOP * HOP
    aec = _aec(1, P)
    res = aec.process(torch.from_numpy(mic[None, :n].copy()), torch.from_numpy(pl[None, :n].copy()))[0].cpu().numpy()
    assert np.array_equal(out[:n], dataio.pcm16_quantise(res).astype(np.float32) / np.float32(32768.0))
    assert np.load(h_path).shape == (P * HOP,) and np.abs(np.load(h_path)).max() > 1e-2
    # another sample rate: an error that names the resampler
    bad = str(tmp_path / 'mic8k.wav')
    dataio.write_wav_pcm16(bad, s['mic'][:L], sr=8000)
    with pytest.raises(SystemExit):
        A.main(['--mic', bad, '--played', pl_path, '--out', out_path])
    assert 'python -m nele_gan_amd.resample' in capsys.readouterr().err
