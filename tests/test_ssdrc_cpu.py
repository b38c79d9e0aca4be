"""CPU: the SSDRC specification as tests/ssdrc_ref.py restates it, pinned by its properties on the toy clean file;
the command line's manifest and argument handling with the enhancer stubbed; the C ABI's argument checks.  The inequality bounds are
those of the issue's prototype run on tests/golden/toy/Train_Clean.wav (1 - 4 kHz share 0.061 -> 0.44 shaped / 0.42 full chain; crest
factor 8.0 -> 5.05 compressed)."""
import csv
import os

import numpy as np
import pytest

import ssdrc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOY = os.path.join(ROOT, 'tests', 'golden', 'toy')


@pytest.fixture(scope='module')
def toy():
    from nele_gan_amd import dataio
    x, sr = dataio.load(os.path.join(TOY, 'Train_Clean.wav'))
    assert sr == 16000
    return x.astype(np.float64)


@pytest.fixture(scope='module')
def chains(toy):
    """the restatement's outputs on the toy file, computed once"""
    return {'shape': R.ssdrc(toy, R.Params(compress=False)), 'compress': R.ssdrc(toy, R.Params(shape=False)), 'full': R.ssdrc(toy)}


def test_unity_gains_are_the_identity(toy):
    assert np.abs(R.shape(toy, gains='unity') - toy).max() <= 1e-12


def test_both_stages_off_is_the_identity(toy):
    assert np.abs(R.ssdrc(toy, R.Params(shape=False, compress=False)) - toy).max() <= 1e-12


def test_equal_energy(toy, chains):
    sx = np.sum(toy ** 2)
    for k, y in chains.items():
        assert abs(np.sum(y ** 2) / sx - 1.0) <= 1e-12, k


def test_shaping_moves_energy_into_1_to_4_khz(toy, chains):
    before, after = R.band_share(toy), R.band_share(chains['shape'])
    print('1-4 kHz share: clean %.3f, shaped %.3f' % (before, after))
    assert before < 0.07 and after > 0.3


def test_compression_lowers_the_crest_factor(toy, chains):
    before, after = R.crest(toy), R.crest(chains['compress'])
    print('crest factor: clean %.2f, compressed %.2f' % (before, after))
    assert before > 7.5 and after < 6.0


def test_full_chain_is_finite_and_shaped(chains):
    y = chains['full']
    assert np.isfinite(y).all() and R.band_share(y) > 0.3


def test_zero_row_gives_zeros():
    for p in (R.Params(), R.Params(shape=False), R.Params(compress=False)):
        y = R.ssdrc(np.zeros(1000), p)
        assert y.shape == (1000,) and not y.any()


def test_reference_authors_file_beside_ours(toy, chains):
    """Reported, not asserted: the parameters behind the reference authors' Train_MultiEnh.wav are unknown."""
    from nele_gan_amd import dataio
    theirs, _ = dataio.load(os.path.join(TOY, 'Train_MultiEnh.wav'))
    print('1-4 kHz share / crest factor: theirs %.3f / %.2f, ours %.3f / %.2f'
          % (R.band_share(theirs), R.crest(theirs), R.band_share(chains['full']), R.crest(chains['full'])))
    assert len(theirs) == len(toy)


# ------------------------------------------------------------------------------------------------ parameters and the C ABI
def test_python_defaults_are_the_library_defaults_and_the_restatement_s():
    from nele_gan_amd import ssdrc
    p = ssdrc.SsdrcParams()
    assert ssdrc.library_defaults() == p
    r = R.Params()
    for f in ('shape', 'compress', 'lifter_q', 'beta', 'preemph', 'attack', 'release', 'e0_ratio', 'knots'):
        assert getattr(p, f) == getattr(r, f), f


def test_invalid_arguments_are_reported_without_a_gpu():
    import ctypes
    from nele_gan_amd import _lib, ssdrc
    lib = _lib.lib
    assert lib.nele_ssdrc(None, None, 0, 0, None, None, None, None) == -1
    assert b'nele_ssdrc' in lib.nele_last_error_string()
    assert lib.nele_ssdrc_shape(None, None, 1, 256, None, None, None, None) == -1
    assert b'nele_ssdrc_shape' in lib.nele_last_error_string()
    assert lib.nele_ssdrc_compress(None, None, 1, 256, None, None, None, None, None) == -1
    assert b'nele_ssdrc_compress' in lib.nele_last_error_string()
    assert lib.nele_ssdrc_ws_bytes(0, 256) == -1
    assert lib.nele_ssdrc_ws_bytes(2, 1024) > 2 * 1024 * 8 * 2
    assert lib.nele_ssdrc_ws_bytes(1, (1 << 30) + 1) == -1 and lib.nele_ssdrc_ws_bytes(65536, 256) == -1
    # a parameter out of range, with every pointer set (host memory is never touched: the check comes first)
    buf = ctypes.create_string_buffer(512)
    aligned = ctypes.c_void_p((ctypes.addressof(buf) + 255) // 256 * 256)
    for bad in (dict(lifter_q=1), dict(attack=1.0), dict(knots=((0.0, 0.0), (-10.0, -5.0))), dict(e0_ratio=0.0),
                dict(knots=((-10.0, float('nan')), (0.0, 0.0))), dict(beta=float('inf'))):
        p = ssdrc.SsdrcParams(**bad).c_struct()
        assert lib.nele_ssdrc(aligned, None, 1, 256, ctypes.byref(p), aligned, aligned, None) == -1, bad
    ok = ssdrc.SsdrcParams().c_struct()
    assert lib.nele_ssdrc(aligned, None, 1, (1 << 30) + 1, ctypes.byref(ok), aligned, aligned, None) == -1
    assert b'Lmax' in lib.nele_last_error_string()
    with pytest.raises(ValueError):
        ssdrc.SsdrcParams(knots=((0.0, 0.0),)).c_struct()


# ------------------------------------------------------------------------------------------------ the command line, enhancer stubbed
def _write_clean(folder, sizes):
    from nele_gan_amd import dataio
    os.makedirs(folder)
    sig = {}
    for k, n in enumerate(sizes):
        x = R.make_signal(n, 10 + k)
        dataio.write_wav_pcm16(os.path.join(folder, 'utt%d.wav' % k), x)
        sig['utt%d.wav' % k] = dataio.load(os.path.join(folder, 'utt%d.wav' % k))[0]
    return sig


def test_cli_writes_files_and_manifest(tmp_path, monkeypatch):
    import torch
    from nele_gan_amd import dataio, ssdrc
    clean_dir, out = str(tmp_path / 'Clean'), str(tmp_path / 'corpus')
    sig = _write_clean(clean_dir, (700, 300, 1024))

    def batches(files, batch, workers, device):              # host tensors in place of dataio.FileBatches (which uploads)
        for k in range(0, len(files), batch):
            rows, lens = dataio.pad_batch([sig[f.split('/')[-1]] for f in files[k:k + batch]])
            yield {'clean': torch.from_numpy(rows), 'lengths': torch.from_numpy(lens), 'lengths_host': lens, 'names': [f.split('/')[-1] for f in files[k:k + batch]]}
    seen = []

    def enhancer(wav, lengths=None, params=None, pcm16=False):
        seen.append(params)
        return wav * 4.0                                      # loud enough to clip
    monkeypatch.setattr(ssdrc, '_batches', batches)
    monkeypatch.setattr(ssdrc, 'ssdrc', enhancer)
    assert ssdrc.main(['--clean', clean_dir, '--out', out, '--batch', '2', '--no-compress']) == 0
    assert seen and all(p == ssdrc.SsdrcParams(compress=False) for p in seen)
    with open(os.path.join(out, 'ssdrc_manifest.csv'), newline='') as fh:
        rows = list(csv.reader(fh))
    assert tuple(rows[0]) == ssdrc.MANIFEST_COLUMNS == ('name', 'samples', 'input_rms', 'peak', 'clipped_samples')
    assert [r[0] for r in rows[1:]] == sorted(sig)
    for r in rows[1:]:
        x = sig[r[0]]
        y, sr = dataio.load(os.path.join(out, 'MultiEnh', r[0]))
        assert sr == 16000 and len(y) == len(x) == int(r[1])
        want = dataio.pcm16_quantise(x * np.float32(4.0))
        assert np.array_equal(np.rint(y * 32768.0).astype(np.int16), want)
        np.testing.assert_allclose(float(r[2]), np.sqrt(np.mean(x.astype(np.float64) ** 2)), rtol=1e-6)
        np.testing.assert_allclose(float(r[3]), 4.0 * np.abs(x).max(), rtol=1e-6)
        clipped = int((np.abs(x * np.float32(4.0)) * np.float32(32767.0) > 32767.5).sum())
        assert int(r[4]) == clipped and clipped > 0


def test_cli_argument_errors(tmp_path, capsys):
    from nele_gan_amd import ssdrc
    empty = tmp_path / 'empty'
    empty.mkdir()
    for argv in (['--out', str(tmp_path)], ['--clean', str(empty), '--out', str(tmp_path)], ['--clean', str(empty), '--out', str(tmp_path), '--batch', '0']):
        with pytest.raises(SystemExit) as e:
            ssdrc.main(argv)
        assert e.value.code == 2
    capsys.readouterr()


def test_other_command_lines_take_the_option(capsys):
    from nele_gan_amd import inference
    with pytest.raises(SystemExit) as e:                     # a baseline is a score: without --score the option is an error, not ignored
        inference.main(['--clean', 'x', '--noise', 'y', '--baseline', 'ssdrc'])
    assert e.value.code == 2 and '--baseline needs --score' in capsys.readouterr().err
    from nele_gan_amd import mix_corpus
    with pytest.raises(ValueError):
        mix_corpus.mix_corpus([], None, '/nonexistent', multienh='other')
    from nele_gan_amd.train_nele import GanTrainer
    with pytest.raises(ValueError):
        GanTrainer.fit(object(), [], None, multienh='other')
