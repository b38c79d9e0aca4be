"""GPU: the stream compressor (nele_gan_amd/drc.py, csrc/drc.hip) against tests/drc_ref.py - the float64 numpy restatement of DESIGN.md
section 23 - its streaming contract (grouping, batch, slots, skipped calls, reset: bitwise, for the output and the two optional
outputs), the offline stage of section 11, CompressedEnhancer around the rule-mode enhancer and inside the echo loop, the figures of
section 23's ssn row and the command line.

Bounds (tests/drc_cases.py): gain and level relative, every sample and hop, under 8 x the all-flipped sensitivity that
tests/test_drc_cpu.py measures on the same inputs (every magnitude a[i] moved one float64 ulp up or down at random), never above 1e-12;
the float32 output within 2^-22 of the reference's peak (one rounding flip).
Measured on an MI355X: at (B, hops) = (1, 40) gain 5.6e-16 (bound 9.6e-15), level bit-equal (3.6e-15); at (3, 264) gain 5.6e-16 / 6.7e-16 /
5.6e-16 (1.0e-14 / 1.0e-14 / 1.1e-14), level bit-equal; every float32 output sample bit-equal to the reference's in both shapes, and to
float32(ssdrc_ref.compress) in the fixed-level run.  The ssn row: SIIB 63.646 and ESTOI 0.3845 for the reference and for the GPU; the
chain on the device 50.79 -> 61.81 and 0.3270 -> 0.3747 for both."""

import numpy as np
import pytest

import drc_cases as K
import ssdrc_ref as S
from drc_ref import HOP, DrcRef

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

SENTINEL = -7.25
WANT = ('gain', 'level')


def _drc(B, **kw):
    from nele_gan_amd.drc import StreamCompressor
    return StreamCompressor(B, **kw)


def feed(drc, xs, group, slots=None):
    """all hops of the given streams through ``drc`` (in ``slots``, default 0 ..), ``group`` hops per call at most
    -> dict: out [n, L] float32; gain [n, L], level [n, L / 256] float64, on the host"""
    slots = list(range(len(xs))) if slots is None else slots
    L = len(xs[0])
    parts = {k: [] for k in ('out',) + WANT}
    for a in range(0, L, group * HOP):
        b = min(L, a + group * HOP)
        X = np.full((drc.S, b - a), np.nan, np.float32)
        act = np.zeros(drc.S, bool)
        for i, s in enumerate(slots):
            X[s], act[s] = xs[i][a:b], True
        got = drc.process(torch.from_numpy(X), active=None if act.all() else act, want=WANT)
        for k, t in zip(('out',) + WANT, got):
            parts[k].append(t[slots].cpu().numpy())
    return {k: np.concatenate(v, axis=1) for k, v in parts.items()}


def cut(d, rows=slice(None), hops=slice(None)):
    """the rows (streams) and hops of every output of a feed()"""
    samples = slice(None if hops.start is None else hops.start * HOP, None if hops.stop is None else hops.stop * HOP)
    return {'out': d['out'][rows, samples], 'gain': d['gain'][rows, samples], 'level': d['level'][rows, hops]}


def same(a, b):
    """the output and the two optional outputs, bit for bit"""
    return all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]) for k in ('out',) + WANT)


def check_parity(tag, got, ref, key):
    """one stream against the reference's run, every sample and hop, under the bounds of these inputs"""
    peak = float(np.abs(ref['out64']).max())
    dev = {'gain': K.rel_dev(got['gain'], ref['gain']), 'level': K.rel_dev(got['level'], ref['level'])}
    bound = K.gpu_bound(key)
    out_dev = float(np.abs(got['out'].astype(np.float64) - ref['out'].astype(np.float64)).max()) / peak
    print('%s: %s, out %.3g of the peak (bound %.3g); %d of %d samples differ'
          % (tag, ', '.join('%s %.3g (bound %.3g)' % (k, dev[k], bound[k]) for k in dev), out_dev, K.OUT_BOUND,
             int((got['out'] != ref['out']).sum()), ref['out'].size))
    assert got['out'].dtype == np.float32 and got['gain'].shape == ref['gain'].shape and got['level'].shape == ref['level'].shape
    assert np.isfinite(got['out']).all() and not got['out'][:HOP].any() and got['out'][HOP:].any()
    for k in dev:
        assert dev[k] <= bound[k], (tag, k, dev[k], bound[k])
    assert out_dev <= K.OUT_BOUND, (tag, out_dev)


def streams(n, hops=40):
    """n different inputs of ``hops`` hops: the speech, circularly shifted"""
    return [K.stream_input(5000 * i, hops) for i in range(n)]


# -------------------------------------------------------------------------------------------------------- parity against the reference
def test_parity_with_the_reference_on_one_stream():
    """(B, hops) = (1, 40), 11 hops per call"""
    key = (0, 40)
    got = feed(_drc(1), [K.stream_input(*key)], 11)
    check_parity('(1, 40)', {k: v[0] for k, v in got.items()}, K.ref_run(*key), key)


def test_parity_with_the_reference_on_three_shifted_streams():
    """(B, hops) = (3, 264), 13 hops per call, the streams shifted against each other by 5000 samples"""
    keys = [k for k in K.SENS_INPUTS if k[1] == 264]
    got = feed(_drc(3), [K.stream_input(*k) for k in keys], 13)
    for i, key in enumerate(keys):
        check_parity('(3, 264) stream %d' % i, {k: v[i] for k, v in got.items()}, K.ref_run(*key), key)


def test_fixed_level_and_no_equaliser_is_the_offline_stage():
    """the fixed-level, equaliser-off run of the speech plus one zero hop against float32(ssdrc_ref.compress): one rounding flip of the peak"""
    s = np.concatenate([K.speech().astype(np.float32), np.zeros(HOP, np.float32)])
    level = S.Params().e0_ratio * S.envelope(s.astype(np.float64)).max()
    got = feed(_drc(1, equalise=False, ref_level=[level]), [s], 24)
    off = S.compress(s.astype(np.float64))[0][:264 * HOP]
    dev = float(np.abs(got['out'][0, HOP:].astype(np.float64) - off.astype(np.float32).astype(np.float64)).max() / np.abs(off).max())
    print('fixed level, no equaliser: %.3g of the peak from float32(ssdrc_ref.compress) (bound %.3g); %d of %d samples differ'
          % (dev, K.OUT_BOUND, int((got['out'][0, HOP:] != off.astype(np.float32)).sum()), off.size))
    assert dev <= K.OUT_BOUND and np.all(got['level'][0, 1:] == level) and got['level'][0, 0] == 0


# ---------------------------------------------------------------------------------------------------------------- bitwise invariances
def test_hop_grouping_and_batch_do_not_change_a_slot():
    xs = streams(5)
    runs = [feed(_drc(1), [xs[3]], group) for group in (1, 7, 40)]
    for r in runs[1:]:
        assert same(r, runs[0])
    assert all(np.isfinite(runs[0][k]).all() for k in runs[0]) and runs[0]['gain'].max() > 2.0 and runs[0]['level'][0, 1:].min() > 0
    # the same stream in slot 3 of B = 5, the other slots busy with their own
    five = feed(_drc(5), xs, 5)
    assert same(cut(five, slice(3, 4)), runs[0])
    assert not np.array_equal(five['out'][2], five['out'][3])


def _record(drc, slot):
    from nele_gan_amd import _lib
    rec = int(_lib.lib.nele_drc_stream_record_bytes())
    header = drc.nbytes - drc.S * rec
    return drc.state[header + slot * rec:header + (slot + 1) * rec].clone()


def test_inactive_slots_are_neither_read_nor_written():
    B, n0, n1 = 3, 18, 6
    xs = streams(B)
    drc = _drc(B)
    feed(drc, [x[:n0 * HOP] for x in xs], 4)
    before = _record(drc, 1)
    assert before.any()
    # a call that skips slot 1: NaN input rows there, sentinel-filled outputs
    X = np.stack([x[n0 * HOP:(n0 + n1) * HOP] for x in xs])
    X[1] = np.nan
    out = (torch.full((B, n1 * HOP), SENTINEL, device='cuda'), torch.full((B, n1 * HOP), SENTINEL, dtype=torch.float64, device='cuda'),
           torch.full((B, n1), SENTINEL, dtype=torch.float64, device='cuda'))
    got = drc.process(torch.from_numpy(X), active=[True, False, True], want=WANT, out=out)
    assert all(g is o for g, o in zip(got, out))
    for t in got:
        assert (t[1] == SENTINEL).all() and not (t[0] == SENTINEL).any() and not (t[2] == SENTINEL).any() and torch.isfinite(t).all()
    assert torch.equal(_record(drc, 1), before)
    assert list(drc.hops) == [n0 + n1, n0, n0 + n1]
    # slot 1 goes on where it was: equal to a run that never saw the skipped call
    later = feed(drc, [xs[1][n0 * HOP:]], 5, slots=[1])
    alone = feed(_drc(1), [xs[1]], 40)
    assert same(later, cut(alone, hops=slice(n0, None)))


def test_reset_restarts_one_slot_and_leaves_the_others():
    B, n0 = 3, 18
    xs = streams(B)
    fresh = feed(_drc(1), [xs[1][:(40 - n0) * HOP]], 22)

    def run(with_reset):
        drc = _drc(B)
        feed(drc, [x[:n0 * HOP] for x in xs], 4)
        if with_reset:
            drc.reset([1])
            assert not _record(drc, 1).any() and _record(drc, 0).any()
            assert list(drc.hops) == [n0, 0, n0]
        x2 = [x[n0 * HOP:] for x in xs]
        if with_reset:
            x2[1] = xs[1][:(40 - n0) * HOP]
        return feed(drc, x2, 7)

    r = run(True)
    assert same(cut(r, slice(1, 2)), fresh)
    r_ = run(False)
    for s in (0, 2):
        assert same(cut(r, slice(s, s + 1)), cut(r_, slice(s, s + 1)))
    assert not np.array_equal(r['out'][1], r_['out'][1])


def test_silence_and_settings_reach_the_kernel():
    z = feed(_drc(1), [np.zeros(40 * HOP, np.float32)], 9)
    assert not z['out'].any() and not z['level'].any() and np.all(z['gain'][0, HOP:] == 1) and not z['gain'][0, :HOP].any()
    x = streams(1, hops=20)[0]
    a, b, c = feed(_drc(1), [x], 20), feed(_drc(1, tau_peak=0.05), [x], 20), feed(_drc(1, equalise=False), [x], 20)
    assert not np.array_equal(a['level'], b['level']) and np.array_equal(a['level'], c['level']) and not np.array_equal(a['out'], c['out'])
    through = feed(_drc(1, ref_level=[0.0]), [x], 20)                         # a level that is not > 0: the input, one hop late
    assert np.array_equal(through['out'][0, HOP:], x[:19 * HOP]) and np.all(through['gain'][0, HOP:] == 1)
    with pytest.raises(ValueError, match='want'):
        _drc(1).process(torch.zeros(1, HOP), want=('gains',))
    o, lv = _drc(1).process(torch.from_numpy(x[None, :2 * HOP].copy()), want='level')
    assert o.shape == (1, 2 * HOP) and lv.shape == (1, 2) and lv.dtype == torch.float64


# --------------------------------------------------------------------------------------------------------- behind the enhancer
def _rt(streams):
    from nele_gan_amd.realtime import RealtimeEnhancer
    from nele_gan_amd.siiopt import SiiOptRule
    return RealtimeEnhancer(rule=SiiOptRule(), streams=streams)


def _two_streams(hops):
    import siiopt_cases as SK
    a, b = SK.scenario('ssn', -5.0), SK.scenario('pink', -5.0)
    cl = np.stack([a['speech'][:hops * HOP], b['speech'][3000:3000 + hops * HOP]])
    ns = np.stack([a['noise'][:hops * HOP], b['noise'][3000:3000 + hops * HOP]])
    return cl, ns


def test_compressed_enhancer_is_the_two_objects_chained_by_hand():
    from nele_gan_amd.drc import CompressedEnhancer
    hops, group, k = 24, 5, 100
    cl, ns = _two_streams(hops + 1)
    chain, rt, drc = CompressedEnhancer(_rt(2), _drc(2)), _rt(2), _drc(2)
    assert chain.S == 2
    for a in range(0, hops * HOP, group * HOP):
        b = min(hops * HOP, a + group * HOP)
        c, v = torch.from_numpy(cl[:, a:b].copy()), torch.from_numpy(ns[:, a:b].copy())
        got = chain.process(c, v)
        assert torch.equal(got, drc.process(rt.process(c, v))), a
    assert got.abs().max().item() > 0
    # finish slot 1 alone, with a tail of k samples: the enhancer's last hop and one zero hop through the compressor
    tc, tn = np.zeros((1, HOP), np.float32), np.zeros((1, HOP), np.float32)
    tc[0, :k], tn[0, :k] = cl[1, hops * HOP:hops * HOP + k], ns[1, hops * HOP:hops * HOP + k]
    two = chain.finish([1], tc, tn, [k])
    last = rt.finish([1], tc, tn, [k])
    full = torch.zeros(2, 2 * HOP, device='cuda')
    full[1, :HOP] = last[0]
    hand = drc.process(full, active=[False, True])
    assert two.shape == (1, 2 * HOP) and torch.equal(two[0], hand[1]) and two[0, HOP:].abs().max().item() > 0
    assert list(chain.drc.hops) == [hops, hops + 2] and chain.rt.finished.tolist() == [False, True]
    chain.reset([1])
    assert list(chain.drc.hops) == [hops, 0] and list(chain.rt.hops) == [hops, 0] and not _record(chain.drc, 1).any() and _record(chain.drc, 0).any()


def test_inside_the_echo_loop_the_canceller_sees_the_compressed_signal():
    from nele_gan_amd.aec import EchoCanceller, EchoCancellingEnhancer
    from nele_gan_amd.drc import CompressedEnhancer
    NH, CALLS = 4, 4                                                              # 16 hops
    cl, ns = _two_streams(NH * CALLS)
    loop = EchoCancellingEnhancer(CompressedEnhancer(_rt(2), _drc(2)), EchoCanceller(2, partitions=4))
    hand_aec, hand_rt, hand_drc = EchoCanceller(2, partitions=4), _rt(2), _drc(2)
    played = torch.zeros(2, NH * HOP, device='cuda')
    for c in range(CALLS):
        cols = slice(c * NH * HOP, (c + 1) * NH * HOP)
        clean = torch.from_numpy(cl[:, cols].copy())
        mic = torch.from_numpy((ns[:, cols] + 0.5 * played.cpu().numpy()).astype(np.float32))       # the noise and an echo of what was played
        out = loop.process(clean, mic)
        rule_out = hand_rt.process(clean, hand_aec.process(mic, played))
        compressed = hand_drc.process(rule_out)
        assert torch.equal(out, compressed) and torch.equal(loop.played, compressed), c
        assert c == 0 or not torch.equal(compressed, rule_out)
        played = compressed
    assert torch.isfinite(out).all() and out.abs().max().item() > 0


def test_figures_of_the_ssn_row_on_the_gpu():
    """Speech-shaped noise at -5 dB.  The table's own row: its input (the reference rule's output) through the GPU compressor against
    the reference's figures.  And the chain on the device: CompressedEnhancer(rule-mode enhancer, compressor), finish included, against
    tests/drc_ref.py on the same enhancer's output.  SIIB within 0.5 %, ESTOI within 0.002."""
    from nele_gan_amd.drc import CompressedEnhancer, compress_file
    row = ('ssn', -5.0, 'rule')
    sp, v, inp = K.row_input(*row)
    ref = K.ref_row(*row)
    got = K.score(sp, v, inp, compress_file(inp.astype(np.float32)))
    print('table row, reference / GPU: SIIB %.3f / %.3f, ESTOI %.4f / %.4f, level %+.3f / %+.3f dB'
          % (ref['siib_out'], got['siib_out'], ref['estoi_out'], got['estoi_out'], ref['level_db'], got['level_db']))
    assert abs(got['siib_out'] / ref['siib_out'] - 1.0) <= K.GPU_SIIB_WITHIN and abs(got['estoi_out'] - ref['estoi_out']) <= K.GPU_ESTOI_WITHIN
    assert got['siib_out'] / got['siib_in'] >= K.MIN_SIIB_RATIO and got['estoi_out'] - got['estoi_in'] >= K.MIN_ESTOI_GAIN
    assert abs(got['level_db']) <= K.MAX_LEVEL_DB
    # the chain on the device, one stream, 24 hops per call
    nh = len(sp) // HOP
    c, n = torch.from_numpy(sp.astype(np.float32)[None]), torch.from_numpy(v.astype(np.float32)[None])
    chain, rt = CompressedEnhancer(_rt(1), _drc(1)), _rt(1)
    zero = np.zeros((1, HOP), np.float32)
    parts, rule_parts = [], []
    for a in range(0, nh * HOP, 24 * HOP):
        parts.append(chain.process(c[:, a:a + 24 * HOP], n[:, a:a + 24 * HOP]))
        rule_parts.append(rt.process(c[:, a:a + 24 * HOP], n[:, a:a + 24 * HOP]))
    out = torch.cat(parts + [chain.finish([0], zero, zero, [0])], dim=1)[0, 2 * HOP:].cpu().numpy()
    fed = torch.cat(rule_parts + [rt.finish([0], zero, zero, [0])], dim=1)[0].cpu().numpy()      # what the compressor was given: the
    rule_out = fed[HOP:]                                                                         # enhancer's zero hop, then its output
    assert out.shape == rule_out.shape == (nh * HOP,) and not fed[:HOP].any()
    r64 = rule_out.astype(np.float64)
    want = DrcRef().run(np.concatenate([fed, zero[0]]))['out'][2 * HOP:]
    fg, fr = K.score(sp, v, r64, out), K.score(sp, v, r64, want)
    print('chain on the device, reference / GPU: SIIB %.3f -> %.3f / %.3f, ESTOI %.4f -> %.4f / %.4f'
          % (fr['siib_in'], fr['siib_out'], fg['siib_out'], fr['estoi_in'], fr['estoi_out'], fg['estoi_out']))
    assert abs(fg['siib_out'] / fr['siib_out'] - 1.0) <= K.GPU_SIIB_WITHIN and abs(fg['estoi_out'] - fr['estoi_out']) <= K.GPU_ESTOI_WITHIN
    assert np.abs(out.astype(np.float64) - want.astype(np.float64)).max() <= K.OUT_BOUND * np.abs(want).max()


# ----------------------------------------------------------------------------------------------------------------------- command line
def test_command_line(tmp_path, capsys):
    from nele_gan_amd import dataio
    from nele_gan_amd import drc as D
    L = 30 * HOP + 100
    in_path, out_path = str(tmp_path / 'in.wav'), str(tmp_path / 'out.wav')
    dataio.write_wav_pcm16(in_path, 8.0 * K.stream_input(0, 31)[:L])              # loud enough for PCM_16 to saturate somewhere
    assert D.main(['--in', in_path, '--out', out_path, '--tau-peak', '2', '--tau-energy', '0.5']) == 0
    said = capsys.readouterr().out
    x, _ = dataio.read_wav(in_path)
    d = np.zeros((1, 32 * HOP), np.float32)
    d[0, :L] = x
    want = _drc(1, tau_peak=2.0, tau_energy=0.5).process(torch.from_numpy(d))[0, HOP:HOP + L].cpu().numpy()
    clipped = int(np.sum(np.abs(want) * np.float32(32767.0) > 32767.5))
    assert 'compressed' in said and ('%d clipped' % clipped) in said and clipped > 0
    out, sr = dataio.read_wav(out_path)
    assert sr == 16000 and out.shape == (L,)
    assert np.array_equal(out, dataio.pcm16_quantise(want).astype(np.float32) / np.float32(32768.0)) and out[L - 100:].any()
