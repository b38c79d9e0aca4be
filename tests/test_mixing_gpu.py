"""GPU: nele_mix_noise_var / NoiseMixer.mix - the SNR that was asked for is the SNR of what comes out (against the reference-generated
active speech levels of tests/golden/p56.npz), the pool segment wraps at its recording's end, rows end in zeros, 'rms' and 'asl' levels
differ by the activity factor, and a row does not depend on its batch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import p56_cases  # noqa: E402
import p56_ref  # noqa: E402

POOL_LENGTHS = np.array([50000, 30011, 7001, 41234], dtype=np.int32)


def _pool():
    rs = np.random.RandomState(11)
    rows = (0.05 * rs.randn(4, 50000)).astype(np.float32)
    rows[1] *= 3.0
    return rows


@pytest.fixture(scope='module')
def setup():
    g, cases = p56_cases.load()
    keep = [i for i in range(len(cases)) if int(g['status'][i]) == 0]
    sig = [cases[i][1] for i in keep]
    L = 131072
    wav = np.zeros((len(sig), L), dtype=np.float32)
    for r, x in enumerate(sig):
        wav[r, :len(x)] = x
    lens = np.array([len(x) for x in sig], dtype=np.int32)
    keys = [cases[i][0] for i in keep]
    return g, keep, torch.from_numpy(wav).cuda(), torch.from_numpy(lens).cuda(), lens, keys


def _mix(level, setup, epoch=1, rows=None):
    from nele_gan_amd.mixing import NoiseMixer
    g, keep, wav, dlens, lens, keys = setup
    m = NoiseMixer((_pool(), POOL_LENGTHS), level=level, seed=7)
    if rows is not None:
        idx = torch.tensor(rows, device='cuda')
        noise = m.mix(wav[idx].contiguous(), dlens[idx].contiguous(), [keys[r] for r in rows], epoch)
    else:
        noise = m.mix(wav, dlens, keys, epoch)
    torch.cuda.synchronize()
    return m, noise.cpu().numpy()


def test_achieved_snr_wraparound_and_zero_tails(setup):
    g, keep, wav, dlens, lens, keys = setup
    m, noise = _mix('asl', setup)
    gain = m.last['gain'].cpu().numpy()
    level = m.last['level'].cpu().numpy()
    assert (m.last['status'].cpu().numpy() == 0).all()
    pool = _pool()
    wrapped = 0
    for b, gi in enumerate(keep):
        n = int(lens[b])
        row, off, snr = int(m.last['rows'][b]), int(m.last['offsets'][b]), float(m.last['snr_db'][b])
        assert p56_cases.rel(level[b], g['asl_msq'][gi]) <= 1e-9
        # the achieved SNR, on the host in float64 from the float32 output and the GOLDEN active speech level: within 1e-5 dB of the target
        # (float32 rounding of the samples moves a mean square by <= 1.2e-7 relative = 5e-7 dB)
        nms = float(np.mean(noise[b, :n].astype(np.float64) ** 2))
        achieved = 10.0 * np.log10(float(g['asl_msq'][gi]) / nms)
        print(keys[b], 'target', snr, 'achieved', achieved, 'row', row, 'offset', off)
        assert abs(achieved - snr) <= 1e-5, (keys[b], achieved, snr)
        # element-wise: a numpy gather (wrapping at the recording's end) times the gain, after the same float32 rounding
        seg = p56_ref.mix_segment(pool[row], POOL_LENGTHS[row], off, n)
        wrapped += int(off + n > POOL_LENGTHS[row])
        assert np.array_equal(noise[b, :n], (gain[b] * seg.astype(np.float64)).astype(np.float32)), keys[b]
        assert p56_cases.rel(gain[b], p56_ref.mix_gain(seg, snr, float(level[b]))) <= 1e-12
        assert not noise[b, n:].any()                                      # zeros behind the row's end
    assert wrapped >= 3


def test_rms_level_differs_from_asl_by_the_activity_factor(setup):
    from nele_gan_amd.asl_P56 import batch_asl_P56
    g, keep, wav, dlens, lens, keys = setup
    ma, _ = _mix('asl', setup)
    mr, _ = _mix('rms', setup)
    act = batch_asl_P56(wav, dlens)['actfact'].cpu().numpy()
    ga, gr = ma.last['gain'].cpu().numpy(), mr.last['gain'].cpu().numpy()
    for b in range(len(keys)):
        # gain^2 is proportional to the speech level: rms / asl = (sq / length) / asl_msq = actfact by definition
        assert p56_cases.rel((gr[b] / ga[b]) ** 2, act[b]) <= 1e-12, keys[b]
        assert abs(10 * np.log10((gr[b] / ga[b]) ** 2) - 10 * np.log10(float(g['actfact'][keep[b]]))) <= 1e-8


def test_rows_do_not_depend_on_the_batch_and_epochs_differ(setup):
    m, whole = _mix('asl', setup)
    for rows in ([3], [5, 0, 2], [7, 6, 5, 4, 3, 2, 1, 0]):
        _, part = _mix('asl', setup, rows=rows)
        for k, r in enumerate(rows):
            assert part[k].tobytes() == whole[r].tobytes()
    _, other = _mix('asl', setup, epoch=2)
    assert sum(int(not np.array_equal(other[b], whole[b])) for b in range(whole.shape[0])) >= whole.shape[0] - 1
    _, again = _mix('asl', setup)
    assert again.tobytes() == whole.tobytes()
    # the mixer's own table of speech levels (second call of one mixer) gives the same bits as measuring again
    from nele_gan_amd.mixing import NoiseMixer
    g, keep, wav, dlens, lens, keys = setup
    m2 = NoiseMixer((_pool(), POOL_LENGTHS), seed=7)
    paths = ['/corpus/Clean/' + k for k in keys]
    m2.mix(wav, dlens, keys, 5, level_keys=paths)
    assert m2.last['meter'] is not None
    cached = m2.mix(wav, dlens, keys, 1, level_keys=paths)
    assert m2.last['meter'] is None and cached.cpu().numpy().tobytes() == whole.tobytes()
    m2.mix(wav, dlens, keys, 1)                                            # without level keys nothing is remembered: measured again
    assert m2.last['meter'] is not None


def test_zero_level_and_zero_noise_give_zero_rows_with_a_status():
    from nele_gan_amd import mixing, synth
    pool = _pool()
    pool[2] = 0.0
    m = mixing.NoiseMixer((pool, POOL_LENGTHS), seed=0)
    clean = np.zeros((3, 20000), dtype=np.float32)
    clean[1] = synth.clean_utterance(3, 20000)
    clean[2] = synth.clean_utterance(4, 20000)
    keys = ['a', 'b', 'c']
    k = 0
    while m.draw(['c'], k)[0][0] != 2:                                     # an epoch in which utterance 'c' draws the silent recording
        k += 1
    noise = m.mix(torch.from_numpy(clean).cuda(), None, keys, k).cpu().numpy()
    st = m.last['status'].cpu().numpy()
    assert st[0] & mixing.ZERO_LEVEL and not noise[0].any()
    from nele_gan_amd import asl_P56
    assert list(np.asarray(m.last['p56_status'].cpu() if hasattr(m.last['p56_status'], 'cpu') else m.last['p56_status'])[[0, 1]]) == [asl_P56.SILENT, 0]
    assert st[2] == mixing.ZERO_NOISE and not noise[2].any()
    assert np.isfinite(noise).all() and np.isfinite(m.last['gain'].cpu().numpy()).all()
    if m.last['rows'][1] != 2:
        assert st[1] == 0 and noise[1].any()


# ------------------------------------------------------------------------------------------------ the training loop on fresh mixes
@pytest.fixture(scope='module')
def corpus(tmp_path_factory):
    """16 synthetic utterances of different lengths (with pre-enhanced examples) and a pool of 4 noise recordings, as wav files"""
    import os
    from nele_gan_amd import dataio, synth
    root = str(tmp_path_factory.mktemp('mixcorpus'))
    rs = np.random.RandomState(4)
    for sub in ('Train/Clean', 'Train/MultiEnh', 'Pool'):
        os.makedirs(os.path.join(root, sub))
    for i in range(16):
        L = int(rs.randint(24000, 32001))
        c = synth.clean_utterance(400 + i, L)
        dataio.write_wav_pcm16('%s/Train/Clean/u%02d.wav' % (root, i), c)
        dataio.write_wav_pcm16('%s/Train/MultiEnh/u%02d.wav' % (root, i), (1.4 * c).astype(np.float32))
    for i, L in enumerate((20000, 48000, 31000, 9000)):                     # shorter and longer than the utterances
        dataio.write_wav_pcm16('%s/Pool/n%d.wav' % (root, i), synth.noise_utterance(50 + i, L, tilt=0.5 + 0.3 * i))
    train = sorted(dataio.get_filepaths(root + '/Train/Clean/'))
    pool = sorted(dataio.get_filepaths(root + '/Pool/'))
    return root, train, pool


def _noise_rows(train, mixer, epoch, batch, **kw):
    from nele_gan_amd import dataio
    fb = dataio.FileBatches(train, None, batch=batch, mixer=mixer, epoch=epoch, **kw)
    out = {}
    try:
        for b in fb:
            assert b['noise'].shape == b['clean'].shape and b['noise_key'][1] == epoch
            nz = b['noise'].cpu().numpy()
            for k, nm in enumerate(b['names']):
                n = int(b['lengths_host'][k])
                assert not nz[k, n:].any()
                out[nm] = nz[k, :n].copy()
    finally:
        fb.close()
    return out


def test_file_batches_mix_per_epoch_and_independently_of_the_batch_size(corpus):
    from nele_gan_amd import dataio
    from nele_gan_amd.mixing import NoiseMixer
    root, train, pool = corpus
    e1 = _noise_rows(train, NoiseMixer(pool, seed=3), 1, 8)
    e2 = _noise_rows(train, NoiseMixer(pool, seed=3), 2, 8)
    assert len(e1) == 16 and all(e1[k].any() for k in e1)
    assert sum(int(not np.array_equal(e1[k], e2[k])) for k in e1) >= 15                  # fresh noise in the next epoch
    b16 = _noise_rows(train, NoiseMixer(pool, seed=3), 1, 16)
    shard = _noise_rows(train[5:11], NoiseMixer(pool, seed=3), 1, 4)                      # a rank's shard, another batch size
    f32 = _noise_rows(train, NoiseMixer(pool, seed=3), 1, 8, int16=False)                 # the per-file float32 reader
    for k in e1:
        assert e1[k].tobytes() == b16[k].tobytes(), k
        assert e1[k].tobytes() == f32[k].tobytes(), k
    for k in shard:
        assert shard[k].tobytes() == e1[k].tobytes(), k
    with pytest.raises(ValueError):
        dataio.FileBatches(train, None)
    with pytest.raises(ValueError):
        dataio.FileBatches(train, root + '/Pool/', mixer=NoiseMixer(pool))


def test_mix_corpus_writes_the_folder_the_loader_reads(corpus):
    import os
    from nele_gan_amd import dataio, mix_corpus
    from nele_gan_amd.mixing import NoiseMixer
    root, train, pool = corpus
    out = root + '/mixed'
    assert mix_corpus.main(['--clean', root + '/Train/Clean', '--noise-pool', root + '/Pool', '--out', out, '--seed', '3', '--batch', '8']) == 0
    want = _noise_rows(train, NoiseMixer(pool, seed=3), 0, 16)
    fb = dataio.FileBatches(train, out + '/Noise/', batch=16)
    try:
        b = fb[0]
        got = b['noise'].cpu().numpy()
        for k, nm in enumerate(b['names']):
            n = int(b['lengths_host'][k])
            assert np.array_equal(got[k, :n], dataio.pcm16_quantise(want[nm]).astype(np.float32) / np.float32(32768.0)), nm    # after PCM_16 rounding
    finally:
        fb.close()
    lines = open(out + '/mix_manifest.csv').read().splitlines()
    assert lines[0] == 'name,pool_file,offset,snr_db,asl_msq,actfact,status,p56_status,clipped_samples' and len(lines) == 17
    f = lines[1].split(',')
    assert f[0] == 'u00.wav' and f[1] in [os.path.basename(p) for p in pool] and 0 < float(f[5]) <= 1.0 and f[6:] == ['0', '0', '0']


def test_fit_with_a_mixer_is_reproducible_and_the_clean_cache_changes_nothing(corpus):
    from nele_gan_amd.mixing import NoiseMixer
    from nele_gan_amd.train_nele import GanTrainer
    root, train, pool = corpus
    seen = {}

    def run(tag, cache, batch=8):
        tr = GanTrainer('siib&haspi&estoi', seed=666)
        mixer = NoiseMixer(pool, seed=3)
        calls = seen.setdefault(tag, [])
        inner = mixer.mix

        def spy(clean, lengths, keys, epoch, **kw):
            nz = inner(clean, lengths, keys, epoch, **kw)
            calls.append((epoch, tuple(keys), nz.clone()))
            return nz
        mixer.mix = spy
        res = tr.fit(train, None, train_enh_path=root + '/Train/MultiEnh/', epochs=2, sampling=16, batch=batch, output_path='%s/out_%s' % (root, tag),
                     pt_dir='%s/chkpt_%s' % (root, tag), log_path='%s/log_%s.txt' % (root, tag), clean_cache=cache, mixer=mixer)
        return tr, res
    a, ra = run('a', False)
    b, rb = run('b', False)
    c, rc = run('c', True)
    assert [r['g_steps'] for r in ra] == [0, 2] and all(r['samples'] == 32 for r in ra)
    by_epoch = {}
    for epoch, keys, nz in seen['a']:
        for k, key in enumerate(keys):
            by_epoch.setdefault(epoch, {})[key] = nz[k]
    assert sorted(by_epoch) == [1, 2] and len(by_epoch[1]) == 16
    differ = sum(int(not torch.equal(by_epoch[1][k][:24000], by_epoch[2][k][:24000])) for k in by_epoch[1])
    assert differ >= 15                                                     # the noise batches of epoch 1 and 2 differ
    assert c.clean_cache.hits > 0
    for other, tag in ((b, 'same seed again'), (c, 'clean cache on')):
        for net in ('G', 'D'):
            for (k, ta), (_, tb) in zip(getattr(a, net).state_dict().items(), getattr(other, net).state_dict().items()):
                assert torch.equal(ta, tb), (tag, net, k)
    assert [float(r['g_loss']) if r['g_loss'] is not None else None for r in ra] == [float(r['g_loss']) if r['g_loss'] is not None else None for r in rc]


def test_one_mixer_over_two_folders_that_share_file_names(tmp_path):
    """Train/Clean/u00.wav and Test/Clean/u00.wav are different signals: through ONE mixer (what GanTrainer.fit does when the validation
    set has no noise files) each row must come out at the SNR drawn for it against ITS OWN active speech level - the mixer remembers
    levels by the clean file's path, never by the name the two share.  Also the public mix() with a key reused for another signal."""
    import os
    from nele_gan_amd import dataio, synth
    from nele_gan_amd.asl_P56 import batch_asl_P56
    from nele_gan_amd.mixing import NoiseMixer
    root = str(tmp_path)
    sig = {}
    for part, scale, start in (('Train', 1.0, 800), ('Test', 0.25, 820)):   # 12 dB apart
        os.makedirs('%s/%s/Clean' % (root, part))
        for i in range(3):
            x = (synth.clean_utterance(start + i, 30000 + 1000 * i) * np.float32(scale)).astype(np.float32)
            dataio.write_wav_pcm16('%s/%s/Clean/u%02d.wav' % (root, part, i), x)
    mixer = NoiseMixer((_pool(), POOL_LENGTHS), seed=5)
    for rnd in range(2):                                                   # second round: every level comes from the mixer's table
        for part in ('Train', 'Test'):
            files = sorted(dataio.get_filepaths('%s/%s/Clean/' % (root, part)))
            fb = dataio.FileBatches(files, None, batch=3, mixer=mixer, epoch=0)
            try:
                b = fb[0]
                assert (b['mix']['meter'] is None) == (rnd == 1)
                level = batch_asl_P56(b['clean'], b['lengths'])['asl_msq'].cpu().numpy()
                nz = b['noise'].cpu().numpy().astype(np.float64)
                for k in range(3):
                    n = int(b['lengths_host'][k])
                    achieved = 10.0 * np.log10(level[k] / np.mean(nz[k, :n] ** 2))
                    print(part, b['names'][k], 'target', b['mix']['snr_db'][k], 'achieved', achieved)
                    assert abs(achieved - float(b['mix']['snr_db'][k])) <= 1e-5, (part, rnd, k, achieved)
            finally:
                fb.close()
    # the public call: the same draw key for two different signals, no level keys -> each measured
    a = torch.from_numpy(synth.clean_utterance(830, 20000)[None]).cuda()
    for x in (a, (0.1 * a).contiguous()):
        nz = mixer.mix(x, None, ['same'], 0).cpu().numpy().astype(np.float64)
        lv = float(batch_asl_P56(x)['asl_msq'][0])
        assert abs(10.0 * np.log10(lv / np.mean(nz ** 2)) - float(mixer.last['snr_db'][0])) <= 1e-5


def test_tag_tells_pools_apart():
    from nele_gan_amd.mixing import NoiseMixer
    p = _pool()
    q = p.copy()
    q[3, 100] += 0.5
    assert NoiseMixer((p, POOL_LENGTHS), seed=1).tag() == NoiseMixer((p.copy(), POOL_LENGTHS), seed=1).tag()
    assert NoiseMixer((p, POOL_LENGTHS), seed=1).tag() != NoiseMixer((q, POOL_LENGTHS), seed=1).tag()
    assert NoiseMixer((p, POOL_LENGTHS), seed=1).tag() != NoiseMixer((p, POOL_LENGTHS - 1), seed=1).tag()
