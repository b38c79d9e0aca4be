"""GPU: the SSDRC kernels (csrc/ssdrc.hip) against the numpy restatement tests/ssdrc_ref.py, stage by stage and as a chain, on the
smallest batch at which each kernel can go wrong; tails, degenerate rows, batch invariance, the switches; the file route against the
on-the-fly route of training; the `ssdrc` baseline of the scoring path."""
import filecmp
import os
import shutil

import numpy as np
import pytest
import torch

import ssdrc_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOY = os.path.join(ROOT, 'tests', 'golden', 'toy')

# max |GPU - ssdrc_ref| as a fraction of the reference row's peak.  Measured on an MI355X over the cases below (the padded batch of five
# rows and the toy clean file), largest value per quantity: stage 1 1.78e-15, stage 2 y 1.04e-15 and e-hat 7.6e-16 (float64 against
# float64), the chain's float32 output 4.24e-08 (the output's rounding to float32: half an ulp is 6e-8 of a value).  The constant is 4 x
# the largest of them; the project's standing claim against its own oracle, 1e-4 (CEILING), is what it may not exceed.
# The float64 quantities of the two stage entry points have a bound of their own, 4 x their largest (stage 1's): with the output's bound a
# stage error of 1e-8 of the peak - a float32 intermediate, a wrong Hilbert tap - would pass, and the stage entry points exist to find it.
CEILING = 1e-4
TOL = 4 * 4.24e-8
TOL64 = 4 * 1.78e-15
assert TOL64 <= TOL <= CEILING
LENS = (1024, 700, 300, 100, 40)       # a multiple of the hop; a partial last frame; < 2 hops; < 1 hop but > the Hilbert half-length; < both windows
LMAX = 1024
PAD = 7.0                              # what the input rows hold behind their lengths: must count as zero


def _toy_clean():
    from nele_gan_amd import dataio
    return dataio.load(os.path.join(TOY, 'Train_Clean.wav'))[0]


@pytest.fixture(scope='module')
def cases():
    """[(name, x [B, L] float32 with PAD behind the rows' ends, lengths, per-row reference dict)] - references computed once, never changed"""
    out = []
    rows = [R.make_signal(n, 3 + k) for k, n in enumerate(LENS)]
    toy = _toy_clean()
    for name, sig, L in (('batch5', rows, LMAX), ('toy', [toy], len(toy))):
        x = np.full((len(sig), L), PAD, dtype=np.float32)
        ref = []
        for k, s in enumerate(sig):
            x[k, :len(s)] = s
            s1 = R.shape(s)
            y2, eh = R.compress(s1)
            ref.append({'s1': s1, 'y2': y2, 'eh': eh, 'full': R.ssdrc(s)})
        out.append((name, x, np.asarray([len(s) for s in sig], dtype=np.int32), ref))
    return out


def _err(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_stages_and_chain_against_the_restatement(cases):
    from nele_gan_amd import ssdrc
    worst = {'shape': 0.0, 'compress': 0.0, 'ehat': 0.0, 'full': 0.0}
    for name, x, lens, ref in cases:
        dx, dl = _dev(x), _dev(lens)
        s1 = ssdrc.ssdrc_shape(dx, dl).cpu().numpy()
        s_in = np.zeros(x.shape, dtype=np.float64)           # stage 2 is fed the REFERENCE's stage-1 output: an error is localised
        for k, r in enumerate(ref):
            s_in[k, :lens[k]] = r['s1']
        y2, eh = (t.cpu().numpy() for t in ssdrc.ssdrc_compress(_dev(s_in), dl))
        full = ssdrc.ssdrc(dx, dl).cpu().numpy()
        assert full.dtype == np.float32
        for k, r in enumerate(ref):
            n = int(lens[k])
            e = {'shape': _err(s1[k, :n], r['s1']), 'compress': _err(y2[k, :n], r['y2']), 'ehat': _err(eh[k, :n], r['eh']),
                 'full': _err(full[k, :n].astype(np.float64), r['full'])}
            print('%s row %d (%d samples): %s' % (name, k, n, ', '.join('%s %.3g' % kv for kv in e.items())))
            for key, v in e.items():
                worst[key] = max(worst[key], v)
            for arr in (s1, y2, eh, full):
                assert not arr[k, n:].any()
    print('largest: ' + ', '.join('%s %.3g' % kv for kv in worst.items()))
    assert worst['full'] <= TOL and all(worst[k] <= TOL64 for k in ('shape', 'compress', 'ehat')), worst


def test_tails_and_degenerate_rows():
    from nele_gan_amd import ssdrc
    x = np.full((3, 1536), PAD, dtype=np.float32)
    lens = np.asarray([1000, 1536, 900], dtype=np.int32)
    x[0, :1000] = 0.0                                        # all zero
    x[1, :] = 0.25                                           # constant: no zero crossing, one dominating bin
    x[2, :900] = R.make_signal(900, 5)
    for p in (ssdrc.SsdrcParams(), ssdrc.SsdrcParams(shape=False), ssdrc.SsdrcParams(compress=False)):
        y = ssdrc.ssdrc(_dev(x), _dev(lens), p).cpu().numpy()
        assert np.isfinite(y).all()
        assert not y[0].any()
        for k in range(3):
            assert not y[k, lens[k]:].any()
        for k in (1, 2):                                     # equal energy (float32 output: 1e-6)
            sx, sy = np.sum(x[k, :lens[k]].astype(np.float64) ** 2), np.sum(y[k].astype(np.float64) ** 2)
            assert abs(sy / sx - 1.0) < 1e-5
    const = ssdrc.ssdrc(_dev(x[1:2])).cpu().numpy()
    assert _err(const[0].astype(np.float64), R.ssdrc(x[1])) <= CEILING     # (not one of the cases TOL was measured on)
    # no lengths: every row is Lmax long
    full = ssdrc.ssdrc(_dev(x[2:3, :900].copy())).cpu().numpy()
    assert np.array_equal(full[0], ssdrc.ssdrc(_dev(x[2:3]), _dev(lens[2:3])).cpu().numpy()[0, :900])
    one = ssdrc.ssdrc(_dev(x[2, :900].copy()))               # [L] in, [L] out
    assert one.shape == (900,) and np.array_equal(one.cpu().numpy(), full[0])


def test_a_row_does_not_depend_on_its_batch(cases):
    from nele_gan_amd import ssdrc
    _, x, lens, ref = cases[0]
    dx, dl = _dev(x), _dev(lens)
    s_in = np.zeros(x.shape, dtype=np.float64)
    for k, r in enumerate(ref):
        s_in[k, :lens[k]] = r['s1']
    full, s1 = ssdrc.ssdrc(dx, dl), ssdrc.ssdrc_shape(dx, dl)
    y2, eh = ssdrc.ssdrc_compress(_dev(s_in), dl)
    for k, n in enumerate(lens.tolist()):
        L1 = (n + 255) // 256 * 256
        x1, l1 = dx[k:k + 1, :L1].contiguous(), dl[k:k + 1]
        assert torch.equal(ssdrc.ssdrc(x1, l1)[0, :n], full[k, :n]), k
        assert torch.equal(ssdrc.ssdrc_shape(x1, l1)[0, :n], s1[k, :n]), k
        a, b = ssdrc.ssdrc_compress(_dev(s_in[k:k + 1, :L1]), l1)
        assert torch.equal(a[0, :n], y2[k, :n]) and torch.equal(b[0, :n], eh[k, :n]), k


def test_both_stages_off_is_the_input_bit_for_bit(cases):
    from nele_gan_amd import ssdrc
    for _, x, lens, _ in cases:
        y = ssdrc.ssdrc(_dev(x), _dev(lens), ssdrc.SsdrcParams(shape=False, compress=False)).cpu().numpy()
        for k, n in enumerate(lens.tolist()):
            assert np.array_equal(y[k, :n].view(np.int32), x[k, :n].view(np.int32)) and not y[k, n:].any()


# ------------------------------------------------------------------------------------------------ routes
def _corpus(root, sizes):
    from nele_gan_amd import dataio
    os.makedirs(os.path.join(root, 'Clean'))
    for k, n in enumerate(sizes):
        dataio.write_wav_pcm16(os.path.join(root, 'Clean', 'utt%d.wav' % k), R.make_signal(n, 20 + k))
    return sorted(dataio.get_filepaths(os.path.join(root, 'Clean') + '/'))


def test_file_route_equals_the_on_the_fly_route(tmp_path):
    from nele_gan_amd import dataio, mix_corpus, mixing, ssdrc
    root = str(tmp_path)
    files = _corpus(root, (5000, 3000, 700))
    assert ssdrc.main(['--clean', os.path.join(root, 'Clean'), '--out', root, '--batch', '2']) == 0
    fb = dataio.FileBatches(files, os.path.join(root, 'Clean') + '/', batch=3, drc_path=os.path.join(root, 'MultiEnh') + '/')
    try:
        b = fb[0]
        assert b['drc_lengths_host'].tolist() == b['lengths_host'].tolist() == [5000, 3000, 700]
        fly = ssdrc.ssdrc(b['clean'], b['lengths'], pcm16=True)
        assert fly.shape == b['drc'].shape and torch.equal(fly, b['drc'])
        assert float(b['drc'].abs().max()) > 0.01
    finally:
        fb.close()
    # mix_corpus --multienh ssdrc writes the same files in its own pass
    other = os.path.join(root, 'mixed')
    rng = np.random.RandomState(1)
    mixer = mixing.NoiseMixer(rng.randn(2, 8000).astype(np.float32) * 0.05)
    mix_corpus.mix_corpus(files, mixer, other, batch=2, multienh='ssdrc')
    for f in files:
        nm = f.split('/')[-1]
        assert filecmp.cmp(os.path.join(root, 'MultiEnh', nm), os.path.join(other, 'MultiEnh', nm), shallow=False)
    assert filecmp.cmp(os.path.join(root, 'ssdrc_manifest.csv'), os.path.join(other, 'ssdrc_manifest.csv'), shallow=False)


def test_run_epoch_makes_the_examples_the_folder_holds(tmp_path):
    """one training batch through run_epoch with the MultiEnh folder, and with multienh='ssdrc' and no folder: the same D items and targets"""
    from nele_gan_amd import dataio, ssdrc
    from nele_gan_amd.train_nele import GanTrainer
    root = str(tmp_path)
    for kind in ('Clean', 'Noise'):
        os.makedirs(os.path.join(root, kind))
        x = dataio.load(os.path.join(TOY, 'Train_%s.wav' % kind))[0]
        dataio.write_wav_pcm16(os.path.join(root, kind, 'a.wav'), x * np.float32(32768.0 / 32767.0))
        dataio.write_wav_pcm16(os.path.join(root, kind, 'b.wav'), x[2000:30000] * np.float32(32768.0 / 32767.0))
    files = sorted(dataio.get_filepaths(os.path.join(root, 'Clean') + '/'))
    ssdrc.ssdrc_corpus(files, root, batch=2)
    tr = GanTrainer('siib&estoi')
    got = []
    tr.d_epoch = lambda samples, batch=32: got.append(samples)

    def epoch(drc_path, multienh, samples):
        tr.multienh = multienh
        fb = dataio.FileBatches(files, os.path.join(root, 'Noise') + '/', batch=2, drc_path=drc_path)
        try:
            assert ('drc' in fb[0]) == (drc_path is not None)
            res = tr.run_epoch(1, fb, ())
        finally:
            fb.close()
        assert res['samples'] == samples
    epoch(os.path.join(root, 'MultiEnh') + '/', None, 4)
    epoch(None, 'ssdrc', 4)
    epoch(None, None, 2)                                        # without either: no pre-enhanced example
    folder, fly = got[0], got[1]
    assert len(folder) == len(fly) == 4
    for a, b in zip(folder, fly):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(folder[0][0], folder[2][0])       # generated and pre-enhanced examples differ
    assert len(got[2]) == 2


def test_fit_with_the_clean_cache_makes_each_example_once(tmp_path, monkeypatch):
    """fit(clean_cache=True, multienh='ssdrc'), no MultiEnh folder, two epochs on two files: every epoch's D samples hold the pre-enhanced
    items, they equal those of a fit from the folder, and the second epoch takes them from the cache - ssdrc runs once per utterance."""
    from nele_gan_amd import dataio, ssdrc
    from nele_gan_amd.train_nele import GanTrainer
    root = str(tmp_path)
    for kind in ('Clean', 'Noise'):
        os.makedirs(os.path.join(root, kind))
        x = dataio.load(os.path.join(TOY, 'Train_%s.wav' % kind))[0]
        dataio.write_wav_pcm16(os.path.join(root, kind, 'a.wav'), x)
        dataio.write_wav_pcm16(os.path.join(root, kind, 'b.wav'), x[2000:30000])
    files = sorted(dataio.get_filepaths(os.path.join(root, 'Clean') + '/'))
    ssdrc.ssdrc_corpus(files, root, batch=2)
    calls = []
    real = ssdrc.ssdrc

    def counted(wav, lengths=None, params=None, pcm16=False):
        calls.append(int(wav.shape[0]))
        return real(wav, lengths, params, pcm16)
    monkeypatch.setattr(ssdrc, 'ssdrc', counted)

    def fit(tag, **kw):
        tr = GanTrainer('siib&estoi')
        got, d_epoch = [], tr.d_epoch

        def keep(samples, batch=32):
            got.append([(it[0].clone(), it[1].clone()) for it in samples])
            return d_epoch(samples, batch=batch)
        tr.d_epoch = keep
        res = tr.fit(files, os.path.join(root, 'Noise') + '/', (), None, epochs=2, sampling=2, batch=2, output_path=os.path.join(root, tag, 'out'),
                     pt_dir=os.path.join(root, tag, 'chkpt'), log_path=os.path.join(root, tag, 'log.txt'), clean_cache=True, **kw)
        assert [r['samples'] for r in res] == [4, 4] and [r['g_steps'] for r in res] == [0, 1]
        return tr, got
    _, folder = fit('folder', train_enh_path=os.path.join(root, 'MultiEnh') + '/')
    assert not calls
    tr, fly = fit('fly', multienh='ssdrc')
    assert tr.multienh == 'ssdrc' and len(tr._drc_cache) == 2
    assert calls == [2]                                      # epoch 1: one batch of two utterances; epoch 2: the cache
    for ep in range(2):
        assert len(folder[ep]) == len(fly[ep]) == 4
        for a, b in zip(folder[ep], fly[ep]):
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # the pre-enhanced items (the last two of an epoch's samples) are the same tensors in both epochs, whatever order the epoch drew
    first = {tuple(it[0].shape): it for it in fly[0][2:]}
    for it in fly[1][2:]:
        assert torch.equal(it[0], first[tuple(it[0].shape)][0]) and torch.equal(it[1], first[tuple(it[0].shape)][1])


def test_ssdrc_baseline_scores(tmp_path):
    """inference --score --baseline ssdrc on two short files: finite scores, one per file (a group per file name), equal to
    eval_metrics.evaluate(clean, SSDRC file, noise) in score_enhanced's own listening condition - anechoic, and no level change of the
    scored file (enh_rms = 0), as every enhanced file is scored there."""
    import io
    from nele_gan_amd import dataio, eval_metrics, inference, ssdrc
    root = str(tmp_path)
    for kind in ('Clean', 'Noise'):
        os.makedirs(os.path.join(root, kind))
        shutil.copy(os.path.join(TOY, 'Train_%s.wav' % kind), os.path.join(root, kind, 'one.wav'))
        shutil.copy(os.path.join(TOY, 'Test_%s.wav' % kind), os.path.join(root, kind, 'two.wav'))
    files = sorted(dataio.get_filepaths(os.path.join(root, 'Clean') + '/'))
    text = io.StringIO()
    res, rooms = inference.score_baseline('ssdrc', os.path.join(root, 'Clean') + '/', os.path.join(root, 'Noise') + '/', files, os.path.join(root, 'out'),
                                          groups=('one', 'two'), out=text)
    assert rooms is None and text.getvalue().startswith('baseline ssdrc\n') and 'SIIB is' in text.getvalue()
    clean_res, _ = inference.score_baseline('clean', os.path.join(root, 'Clean') + '/', os.path.join(root, 'Noise') + '/', files, os.path.join(root, 'out'),
                                            groups=('one', 'two'), out=io.StringIO())
    for g in ('one', 'two'):
        c = dataio.load(os.path.join(root, 'Clean', g + '.wav'))[0]
        v = dataio.load(os.path.join(root, 'Noise', g + '.wav'))[0]
        enh = ssdrc.ssdrc(_dev(c), pcm16=True)
        want = eval_metrics.evaluate(c, enh, v, enh_rms=0.0)
        assert res[g]['files'] == 1
        for m in ('siib', 'haspi', 'estoi'):
            assert np.isfinite(res[g][m])
            np.testing.assert_allclose(res[g][m], float(want[m][0]), rtol=1e-6)
        assert any(res[g][m] != clean_res[g][m] for m in ('siib', 'haspi', 'estoi'))
