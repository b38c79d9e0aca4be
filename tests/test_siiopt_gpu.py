"""GPU: the SII-optimal band gains (nele_gan_amd/siiopt.py, csrc/siiopt.h, siiopt.hip, rt_rule_kernel of realtime.hip) against the
float64 reference tests/siiopt_ref.py on the scenarios and bounds of tests/siiopt_cases.py: the offline mask, the offline chain with the
rule in the generator's place, the real-time rule hop (bit-identical to the offline kernel), on-device scoring and the training hook."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import siiopt_cases as S  # noqa: E402
import siiopt_ref as R  # noqa: E402

HERE = os.path.dirname(__file__)
TOY = os.path.join(HERE, 'golden', 'toy')
HOP = 256


def _rule(**kw):
    from nele_gan_amd.siiopt import SiiOptRule
    return SiiOptRule(**kw)


def _gpu_mask(cb, nb, **kw):
    """cb, nb [B, T, 64] numpy -> the kernel's mask, numpy"""
    m = _rule(**kw)(torch.from_numpy(np.ascontiguousarray(cb)).cuda(), torch.from_numpy(np.ascontiguousarray(nb)).cuda())
    return m.cpu().numpy()


def _close(got, ref):
    """the GPU bound: relative 1e-6 on every mask value, none excluded"""
    assert got.shape == ref.shape and got.dtype == np.float32
    assert np.all(np.isfinite(got))
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64)) / ref.astype(np.float64)
    print('largest relative deviation %.3g' % err.max())
    assert err.max() <= S.GPU_RTOL, err.max()


@pytest.mark.parametrize('B,T', [(1, 1), (1, 2), (3, 40), (2, 264)])
def test_offline_mask_against_the_reference(B, T):
    rows = S.parity_inputs()
    cb = np.stack([rows[b][0][:T] for b in range(B)]).copy()
    nb = np.stack([rows[b][1][:T] for b in range(B)]).copy()
    if (B, T) == (3, 40):                                          # frame counts 40 / 17 / 1: zero features behind a row's end
        for b, n in enumerate((40, 17, 1)):
            cb[b, n:] = 0.0
            nb[b, n:] = 0.0
    got = _gpu_mask(cb, nb)
    ref = np.stack([R.mask(cb[b], nb[b]) for b in range(B)])
    _close(got, ref)


def _made_up_rows():
    f = S.features('pink', -5.0)
    T = 12
    a_cb, a_nb = f['cb'][60:60 + T].copy(), f['nb'][60:60 + T].copy()
    a_cb[0] = 0.0                                                  # an all-zero clean frame first
    b_cb, b_nb = f['cb'][100:100 + T].copy(), f['nb'][100:100 + T].copy()
    b_nb[1, ::3] = np.nan                                          # NaN and zero noise features
    b_nb[2] = np.nan
    b_nb[3, 1::2] = 0.0
    b_nb[4] = 0.0
    c_cb = f['cb'][140:140 + T].copy()
    c_nb = (c_cb * np.float32(10.0)).astype(np.float32)            # noise 1e6 times the speech in every band
    return np.stack([a_cb, b_cb, c_cb]), np.stack([a_nb, b_nb, c_nb])


def test_made_up_rows():
    cb, nb = _made_up_rows()
    rng = np.random.default_rng(3)
    holes = R.band_importance() + 0.01
    holes[rng.uniform(size=64) < 0.3] = 0.0
    one_hot = np.zeros(64)
    one_hot[20] = 1.0
    for gamma in (None, holes / holes.sum(), one_hot):
        for strength in (1.0, 0.5):
            for lam in (0.0, 0.98):
                got = _gpu_mask(cb, nb, importance=gamma, strength=strength, lam=lam)
                ref = np.stack([R.mask(cb[b], nb[b], gamma=gamma, strength=strength, lam=lam) for b in range(3)])
                _close(got, ref)
                assert np.all(got[0, 0] == 1.0)                    # nothing to redistribute yet: the mask is 1
                lim = np.float32(np.exp(strength * R.LOGMAX))
                assert got.max() <= lim * (1 + 1e-6) and got.min() >= (1 / lim) * (1 - 1e-6)


def test_a_rows_mask_does_not_depend_on_the_batch():
    rows = S.parity_inputs()
    cb, nb = rows[1][0][:150], rows[1][1][:150]
    alone = _gpu_mask(cb[None], nb[None])[0]
    rng = np.random.default_rng(9)
    for pos in (0, 3, 6):
        CB = (rng.uniform(0.05, 1.0, (7, 150, 64))).astype(np.float32)
        NB = (rng.uniform(0.05, 1.0, (7, 150, 64))).astype(np.float32)
        CB[pos], NB[pos] = cb, nb
        assert np.array_equal(_gpu_mask(CB, NB)[pos].view(np.int32), alone.view(np.int32)), pos


@pytest.fixture(scope='module')
def batch():
    """two scenarios side by side, the second one cut short: clean, noise [2, L] on the device and the lengths"""
    a, b = S.scenario('ssn', -5.0), S.scenario('white', 0.0)
    L = len(a['speech'])
    n1 = 20000
    c = np.stack([a['speech'], np.concatenate([b['speech'][:n1], np.zeros(L - n1, np.float32)])])
    v = np.stack([a['noise'], np.concatenate([b['noise'][:n1], np.zeros(L - n1, np.float32)])])
    return torch.from_numpy(c).cuda(), torch.from_numpy(v).cuda(), torch.tensor([L, n1], dtype=torch.int32).cuda()


@pytest.mark.parametrize('norm', ['utterance', 'prefix'])
def test_offline_chain_against_the_reference(batch, norm):
    """Enhancer(G=SiiOptRule()) on the device's own features against the reference mask and normalisation through
    oracle.features.resyn, at the tolerance gain_istft's own tests use (tests/test_features_gpu.py: 5e-6 of the peak)"""
    from nele_gan_amd import audio_util as au
    from nele_gan_amd.inference import Enhancer
    from oracle import features as F
    c, v, lens = batch
    e = Enhancer(G=_rule(), norm=norm)
    y = e.enhance(c, v, pcm16=False, lengths=lens, rms_target=0).cpu().numpy()
    frames = au.frames_of(lens)
    spec, band = au.stft_band(c, 1.0 / 6, lengths=lens)
    nband = au.noise_band(v, 1.0 / 6, lengths=lens, frames=frames)
    for b, n in enumerate(lens.cpu().tolist()):
        T = 1 + n // HOP
        cb, nb = band[b, :T].cpu().numpy(), nband[b, :T].cpu().numpy()
        m = R.mask(cb, nb)
        a2 = (R.alpha2_utterance if norm == 'utterance' else R.alpha2_prefix)(m, cb)
        ref = F.resyn(spec[b, :T].cpu().numpy().T, a2)
        assert len(ref) == HOP * (n // HOP)
        np.testing.assert_allclose(y[b, :len(ref)], ref, atol=5e-6 * np.abs(ref).max(), rtol=0)
        assert not y[b, len(ref):].any()
    # the whole chain with its final rms and PCM_16: enhance_stream equals enhance bit for bit
    one = e.enhance(c, v, lengths=lens)
    assert abs(float(one[0].double().pow(2).mean().sqrt()) - 0.03) < 1e-4
    streamed = list(e.enhance_stream([(c, v, lens), (c[:1], v[:1]), (c, v, lens)], inflight=2))
    assert torch.equal(streamed[0], one) and torch.equal(streamed[2], one)
    assert torch.equal(streamed[1], e.enhance(c[:1], v[:1]))


# ------------------------------------------------------------------------------------------------ real time
@pytest.fixture(scope='module')
def utts():
    """three streams: the ssn scenario (264 hops, no tail), the pink one cut to 100 hops + 40 samples, 30 hops + 255 samples of the white"""
    a, b, c = S.scenario('ssn', -5.0), S.scenario('pink', -5.0), S.scenario('white', 0.0)
    cl = [a['speech'], b['speech'][:100 * HOP + 40], c['speech'][5000:5000 + 30 * HOP + 255]]
    ns = [a['noise'], b['noise'][:100 * HOP + 40], c['noise'][5000:5000 + 30 * HOP + 255]]
    return [np.ascontiguousarray(x) for x in cl], [np.ascontiguousarray(x) for x in ns]


def _rt(streams, rule=None, norm='prefix'):
    from nele_gan_amd.realtime import RealtimeEnhancer
    return RealtimeEnhancer(rule=rule or _rule(), streams=streams, norm=norm)


def _stream_all(*a, **kw):
    from test_realtime_gpu import stream_all
    return stream_all(*a, **kw)


@pytest.fixture(scope='module')
def rt_run(utts):
    from nele_gan_amd.realtime import RealtimeDebug
    cl, ns = utts
    T = 1 + max(len(c) for c in cl) // HOP
    rt = _rt(len(cl))
    dbg = RealtimeDebug(len(cl), T)
    ys = _stream_all(rt, cl, ns, 7, dbg)
    torch.cuda.synchronize()
    return rt, dbg, ys


def test_streamed_mask_is_the_offline_kernels_bit_for_bit(utts, rt_run):
    _, dbg, _ = rt_run
    cl, _ = utts
    rule = _rule()
    for i, c in enumerate(cl):
        T = 1 + len(c) // HOP
        off = rule(dbg.band[i:i + 1, :T].contiguous(), dbg.noise[i:i + 1, :T].contiguous())[0]
        assert torch.equal(off.view(torch.int32), dbg.mask[i, :T].view(torch.int32)), i
        ref = R.mask(dbg.band[i, :T].cpu().numpy(), dbg.noise[i, :T].cpu().numpy())
        _close(dbg.mask[i, :T].cpu().numpy(), ref)


def test_streamed_output_equals_the_offline_prefix_chain(utts, rt_run):
    from nele_gan_amd.inference import Enhancer
    rt, _, ys = rt_run
    cl, ns = utts
    e = Enhancer(G=_rule(), norm='prefix')
    for i, (c, n) in enumerate(zip(cl, ns)):
        ref = e.enhance(torch.from_numpy(c).cuda()[None], torch.from_numpy(n).cuda()[None], pcm16=False, rms_target=0)[0]
        assert ys[i].shape == ref.shape == (HOP * (len(c) // HOP),)
        assert rt.emitted[i] == HOP * (len(c) // HOP) and rt.finished[i]
        assert (ys[i] - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()


def test_hop_grouping_and_neighbours_do_not_change_a_slot(utts, rt_run):
    _, _, ys = rt_run
    cl, ns = utts
    c, v = cl[1], ns[1]
    for group in (1, 10 ** 6):                                   # rt_run fed 7 hops a call
        y = _stream_all(_rt(1), [c], [v], group)[0]
        assert torch.equal(y, ys[1]), group
    # slot 3 of 5, the other slots busy with other audio
    others = [cl[0][:len(c)], cl[0][3000:3000 + len(c)], cl[0][7000:7000 + len(c)], cl[0][9000:9000 + len(c)]]
    onoise = [ns[0][:len(c)], ns[0][3000:3000 + len(c)], ns[0][7000:7000 + len(c)], ns[0][9000:9000 + len(c)]]
    y5 = _stream_all(_rt(5), others[:3] + [c] + others[3:], onoise[:3] + [v] + onoise[3:], 4)[3]
    assert torch.equal(y5, ys[1])


def test_reset_restarts_one_slot_and_leaves_the_other(utts, rt_run):
    _, _, ys = rt_run
    cl, ns = utts
    c, v = cl[2], ns[2]
    rt = _rt(2)
    junk = torch.from_numpy(np.stack([cl[0][:10 * HOP], cl[0][:10 * HOP]]))
    jn = torch.from_numpy(np.stack([ns[0][:10 * HOP], ns[0][:10 * HOP]]))
    rt.process(junk, jn)
    rt.reset([1])
    assert rt.hops.tolist() == [10, 0]
    nh = len(c) // HOP
    C = np.stack([cl[0][10 * HOP:(10 + nh) * HOP], c[:nh * HOP]])
    N = np.stack([ns[0][10 * HOP:(10 + nh) * HOP], v[:nh * HOP]])
    out = rt.process(torch.from_numpy(C), torch.from_numpy(N))
    k = len(c) - nh * HOP
    tc, tn = np.zeros((1, HOP), np.float32), np.zeros((1, HOP), np.float32)
    tc[0, :k], tn[0, :k] = c[nh * HOP:], v[nh * HOP:]
    last = rt.finish([1], tc, tn, [k])
    assert torch.equal(torch.cat([out[1], last[0]])[HOP:], ys[2])            # slot 1: as a fresh stream
    assert torch.equal(out[0], ys[0][9 * HOP:(9 + nh) * HOP])                # slot 0 (output hops 9 ..): went on undisturbed


def test_a_start_on_exact_zeros_stays_finite(utts):
    from nele_gan_amd.realtime import RealtimeDebug
    cl, ns = utts
    rt = _rt(1)
    dbg = RealtimeDebug(1, 60)
    z = torch.zeros(1, 40 * HOP)
    out0 = rt.process(z, z, debug=dbg)
    out1 = rt.process(torch.from_numpy(cl[0][None, :19 * HOP].copy()), torch.from_numpy(ns[0][None, :19 * HOP].copy()), debug=dbg)
    torch.cuda.synchronize()
    assert torch.isfinite(out0).all() and torch.isfinite(out1).all() and out0.abs().max().item() == 0.0
    assert out1.abs().max().item() > 1e-3
    m = dbg.mask[0, :59]
    assert torch.isfinite(m).all() and torch.isfinite(dbg.alpha2[0, :59]).all()
    assert (m[:40] == 1.0).all()                                  # nothing to redistribute: the mask is 1


def test_fixed_normalisation_scales_the_mask(utts):
    from nele_gan_amd.realtime import RealtimeDebug
    cl, ns = utts
    rt = _rt(1, norm=torch.tensor([0.25]))
    dbg = RealtimeDebug(1, 12)
    rt.process(torch.from_numpy(cl[0][None, :10 * HOP].copy()), torch.from_numpy(ns[0][None, :10 * HOP].copy()), debug=dbg)
    assert torch.equal(dbg.alpha2[0, :10], dbg.mask[0, :10] * 0.25)


def test_the_wrappers_take_a_rule_enhancer_as_it_is(utts):
    """the duplex chain (echo canceller, enhancer, uplink suppressor) and a 48 kHz device around RealtimeEnhancer(rule=...): with nothing
    played back yet the canceller passes the microphone through, so the loop's first call is the bare enhancer's"""
    from nele_gan_amd import streamrate
    from nele_gan_amd.aec import EchoCanceller, EchoCancellingEnhancer
    from nele_gan_amd.ns import DuplexEnhancer, NoiseSuppressor
    cl, ns = utts
    c = torch.from_numpy(cl[0][None, :8 * HOP].copy())
    v = torch.from_numpy(ns[0][None, :8 * HOP].copy())
    bare = _rt(1).process(c, v)
    duplex = DuplexEnhancer(EchoCancellingEnhancer(_rt(1), EchoCanceller(streams=1, partitions=4)), NoiseSuppressor(streams=1))
    out, uplink = duplex.process(c, v)
    assert out.shape == uplink.shape == (1, 8 * HOP) and torch.isfinite(out).all() and torch.isfinite(uplink).all()
    assert (out - bare).abs().max().item() <= 1e-4 * bare.abs().max().item() and bare.abs().max().item() > 1e-3
    wide = streamrate.adapt(_rt(1), 48000)
    c48 = torch.zeros(1, 8 * 768)
    c48[0, ::3] = c[0]
    y = wide.process(c48, torch.zeros(1, 8 * 768))
    assert y.shape == (1, 8 * 768) and torch.isfinite(y).all()


# ------------------------------------------------------------------------------------------------ scoring, training
def test_on_device_siib_meets_the_cpu_bound():
    """speech-shaped noise at -5 dB through Enhancer(G=SiiOptRule()), scored with the project's own SIIB on the GPU"""
    from nele_gan_amd import metrics
    from nele_gan_amd.inference import Enhancer
    s = S.scenario('ssn', -5.0)
    c, v = torch.from_numpy(s['speech']).cuda()[None], torch.from_numpy(s['noise']).cuda()[None]
    y = Enhancer(G=_rule()).enhance(c, v, pcm16=False)[0].cpu().numpy().astype(np.float64)
    x, n = s['speech'].astype(np.float64), s['noise'].astype(np.float64)
    before = metrics.SIIB_Wrapper_raw_harvard(x, x + n, 16000)
    after = metrics.SIIB_Wrapper_raw_harvard(x[:len(y)], y + n[:len(y)], 16000)
    print('raw SIIB on the device: %.2f -> %.2f (x %.3f); the reference: %.2f -> %.2f' % ((before, after, after / before) + S.MEASURED['ssn'][:2]))
    assert after / before >= S.MIN_SIIB_RATIO['ssn']


def test_fit_makes_the_examples_the_corpus_tool_writes(tmp_path):
    """fit(multienh='siiopt'), one tiny epoch on the toy corpus: its pre-enhanced D items and targets are those of a fit from the folder
    python -m nele_gan_amd.siiopt writes"""
    from nele_gan_amd import dataio, siiopt
    from nele_gan_amd.train_nele import GanTrainer
    root = str(tmp_path)
    for kind in ('Clean', 'Noise'):
        os.makedirs(os.path.join(root, kind))
        x = dataio.load(os.path.join(TOY, 'Train_%s.wav' % kind))[0]
        dataio.write_wav_pcm16(os.path.join(root, kind, 'a.wav'), x)
        dataio.write_wav_pcm16(os.path.join(root, kind, 'b.wav'), x[2000:30000])
    files = sorted(dataio.get_filepaths(os.path.join(root, 'Clean') + '/'))
    assert siiopt.main(['--clean', os.path.join(root, 'Clean'), '--noise', os.path.join(root, 'Noise'), '--out', root, '--batch', '2']) == 0
    assert sorted(os.listdir(os.path.join(root, 'MultiEnh'))) == ['a.wav', 'b.wav']
    # the files hold the rule's output for the batch's rows after the PCM_16 round trip
    fb = dataio.FileBatches(files, os.path.join(root, 'Noise') + '/', batch=2, drc_path=os.path.join(root, 'MultiEnh') + '/')
    try:
        b = fb[0]
        fly, n = siiopt.pre_enhance(b['clean'], b['noise'], b['lengths'])
        assert n.cpu().tolist() == list(b['drc_lengths_host']) == [HOP * (int(v) // HOP) for v in b['lengths_host']]
        assert fly.shape == b['drc'].shape and torch.equal(fly, b['drc']) and float(fly.abs().max()) > 0.01
    finally:
        fb.close()

    def fit(tag, **kw):
        tr = GanTrainer('siib&estoi')
        got, d_epoch = [], tr.d_epoch

        def keep(samples, batch=32):
            got.append([(it[0].clone(), it[1].clone()) for it in samples])
            return d_epoch(samples, batch=batch)
        tr.d_epoch = keep
        res = tr.fit(files, os.path.join(root, 'Noise') + '/', (), None, epochs=1, sampling=2, batch=2, output_path=os.path.join(root, tag, 'out'),
                     pt_dir=os.path.join(root, tag, 'chkpt'), log_path=os.path.join(root, tag, 'log.txt'), **kw)
        assert [r['samples'] for r in res] == [4]
        return tr, got
    _, folder = fit('folder', train_enh_path=os.path.join(root, 'MultiEnh') + '/')
    tr, fly = fit('fly', multienh='siiopt')
    assert tr.multienh == 'siiopt' and len(folder[0]) == len(fly[0]) == 4
    for a, b in zip(folder[0], fly[0]):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
