"""GPU: the quality discriminator trained on HASQI v2 targets computed on the device (quality.HasqiScorer) through the epoch driver -
no PESQ / ViSQOL program registered anywhere."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
L = 16384


def _batches():
    """Two training batches of two 1 s utterances with a pre-enhanced example each (a fixed spectral tilt of the clean signal)."""
    from nele_gan_amd import synth
    c, v = synth.batch(4, L, start=900)
    drc = np.stack([np.convolve(r, [1.0, -0.6], mode='same') for r in c]).astype(np.float32)
    out = []
    for k in (0, 2):
        out.append({'clean': torch.from_numpy(c[k:k + 2]).cuda(), 'noise': torch.from_numpy(v[k:k + 2]).cuda(), 'drc': torch.from_numpy(drc[k:k + 2]).cuda(),
                    'names': ['utt%d.wav' % k, 'utt%d.wav' % (k + 1)], 'ids': torch.tensor([100 + k, 101 + k], device='cuda')})
    return out


def _trainer(cache=False, metrics='estoi', stream=None):
    from nele_gan_amd import quality
    from nele_gan_amd.train_nele import GanTrainer
    quality.clear_backends()
    tr = GanTrainer(metrics, use_quality=True, quality_scorer=quality.HasqiScorer())
    if stream is not None:
        tr.quality_stream = stream
    if cache:
        tr.enable_clean_cache(1 << 30)
    return tr


def _quality_targets(items):
    return sorted(tuple(float(v) for v in it[2].cpu().numpy()) for it in items)


def _two_epochs(tr, train):
    per_epoch = []
    for ep in (1, 2):
        random.seed(500 + ep)
        n0 = len(tr.history)
        out = tr.run_epoch(ep, train, train[:1], d_batch=4)
        per_epoch.append((out, _quality_targets(tr.history[n0:])))
    return per_epoch


def test_two_epochs_train_d_qua_on_hasqi_targets_with_and_without_the_cache(tmp_path):
    from nele_gan_amd import metrics as mt
    train = _batches()
    tr = _trainer()
    w0 = tr.D_Qua.layers[4].weight_orig.detach().clone()
    # epoch 1 has no G-step: the generated examples are those of the untrained generator, computable beforehand
    want = []
    for b in train:
        f = tr.features(b['clean'], b['noise'])
        enh = tr.generate(f['clean_band'], f['noise_band'], f['clean_spec'])
        for ex in (enh, b['drc']):
            q = mt.batch_hasqi(b['clean'], ex[:, :L].contiguous(), lengths=[L, L], noise='utterance', seed=0, utt_ids=b['ids'])
            assert bool(torch.isfinite(q).all()) and bool(((q[:, 1:3] >= 0) & (q[:, 1:3] <= 1)).all())
            want += [tuple(float(v) for v in r) for r in q[:, 1:3].float().cpu().numpy()]
    (out1, q1), (out2, q2) = _two_epochs(tr, train)
    assert out1['samples'] == 8 and out1['d_steps'] == 6 and tr.optimizer_dqua.step_count == 12
    assert q1 == sorted(want)                                               # bit for bit
    assert not torch.equal(w0, tr.D_Qua.layers[4].weight_orig.detach()) and np.isfinite(float(tr.last_loss_qua))
    assert all(v == 0 for v in out2['status'].values())
    v = out2['valid']                                                       # raw Combined / Nonlin / Linear of the validation pass
    assert 0.0 < v['hasqi'] <= 1.0 and v['hasqi'] <= min(v['hasqi_nonlin'], v['hasqi_linear']) + 1e-12
    # the same two epochs with the clean-signal cache on: targets and weights bit-identical, the clean halves come from the cache
    tc = _trainer(cache=True)
    (_c1, qc1), (_c2, qc2) = _two_epochs(tc, train)
    assert qc1 == q1 and qc2 == q2
    for mod_a, mod_b in ((tr.G, tc.G), (tr.D, tc.D), (tr.D_Qua, tc.D_Qua)):
        for (k, ta), (_, tb) in zip(mod_a.state_dict().items(), mod_b.state_dict().items()):
            assert torch.equal(ta, tb), k
    st = tc.clean_cache.stats()
    assert any(kind == 'hasqi' for (kind, _g) in tc.clean_cache.pools) and st['hits'] >= 2, st    # ESTOI has no clean half: the hits are HASQI's
    # checkpoints say what D_Qua was trained on, and a trainer that scores the other kind of target refuses them
    from nele_gan_amd import quality
    from nele_gan_amd.train_nele import GanTrainer
    ck = str(tmp_path / 'q.pt')
    tr.save_checkpoint(ck)
    assert torch.load(ck, map_location='cpu')['quality-targets'] == 'hasqi'
    again = _trainer()
    again.load_checkpoint(ck)
    assert torch.equal(again.D_Qua.state_dict()['layers.4.weight_orig'], tr.D_Qua.state_dict()['layers.4.weight_orig'])
    again.save_checkpoint(ck)
    assert torch.load(ck, map_location='cpu')['quality-targets'] == 'hasqi'
    with pytest.raises(ValueError):
        GanTrainer('estoi', use_quality=True, quality_scorer=quality.Scorer()).load_checkpoint(ck)


def test_a_silent_generated_row_is_counted_and_check_status_raises():
    train = _batches()[:1]
    tr = _trainer()
    gen = tr.generate

    def silent_row(*a, **k):
        enh = gen(*a, **k)
        enh[1] = 0.0
        return enh
    tr.generate = silent_row
    tr.run_epoch(1, train, (), d_batch=4, check=False)
    st = tr.check_status(raise_on_error=False)
    assert st['hasqi_below_threshold'] == 1 and st['skipped_dqua_steps'] >= 1, st
    with pytest.raises(RuntimeError):
        tr.check_status()


def _regroup(batches, order):
    """The utterances of ``batches`` as new batches of two in ``order`` - without 'ids': what dataio.FileBatches / fit hand over"""
    rows = [(b, r) for b in batches for r in range(2)]
    out = []
    for k in range(0, len(order), 2):
        pick = [rows[i] for i in order[k:k + 2]]
        nb = {key: torch.stack([b[key][r] for b, r in pick]) for key in ('clean', 'noise', 'drc')}
        nb['names'] = [b['names'][r] for b, r in pick]
        out.append(nb)
    return out


@pytest.mark.parametrize('stream', ['estoi', 'haspi'])
def test_batches_without_ids_redrawn_every_epoch_on_a_metric_stream(stream):
    """Two metrics: the HASQI chain runs on the side stream ``quality_stream`` names.  The batches carry names but no ids and are drawn
    in another order in epoch 2, as fit does: the per-utterance noise follows the utterance's key, so an utterance's target does not
    depend on its row, and the cached run equals the uncached one bit for bit."""
    from nele_gan_amd import metrics as mt
    from nele_gan_amd import quality
    base = _batches()
    epochs = [_regroup(base, [0, 1, 2, 3]), _regroup(base, [3, 0, 2, 1])]
    runs = []
    for cache in (False, True):
        tr = _trainer(cache=cache, metrics='haspi&estoi', stream=stream)
        want = []
        if not cache:                                                       # epoch 1: the untrained generator's examples, computable beforehand
            for b in epochs[0]:
                f = tr.features(b['clean'], b['noise'])
                enh = tr.generate(f['clean_band'], f['noise_band'], f['clean_spec'])
                for ex in (enh, b['drc']):
                    q = mt.batch_hasqi(b['clean'], ex[:, :L].contiguous(), lengths=[L, L], noise='utterance', seed=0,
                                       utt_ids=quality.utterance_ids(b['names']))
                    want += [tuple(float(v) for v in r) for r in q[:, 1:3].float().cpu().numpy()]
        per_epoch = []
        for ep, train in enumerate(epochs, start=1):
            random.seed(700 + ep)
            n0 = len(tr.history)
            out = tr.run_epoch(ep, train, (), d_batch=4)
            assert all(v == 0 for v in out['status'].values()), out['status']
            per_epoch.append(_quality_targets(tr.history[n0:]))
        if not cache:
            assert per_epoch[0] == sorted(want)                             # bit for bit, from the side stream
        runs.append((tr, per_epoch))
    (ta, qa), (tb, qb) = runs
    assert qa == qb
    # the pre-enhanced examples do not change with the epoch: scored again at other rows in the uncached run, their targets are the same
    drc1 = set(qa[0]) & set(qa[1])
    assert len(drc1) >= 4, (qa[0], qa[1])
    for mod_a, mod_b in ((ta.G, tb.G), (ta.D, tb.D), (ta.D_Qua, tb.D_Qua)):
        for (k, va), (_, vb) in zip(mod_a.state_dict().items(), mod_b.state_dict().items()):
            assert torch.equal(va, vb), k
    assert any(kind == 'hasqi' for (kind, _g) in tb.clean_cache.pools)


def test_score_quality_reports_hasqi_per_noise_group(tmp_path):
    """inference.score_quality: groups by name, each pair cut to the shorter file, files with an undefined score left out of the mean."""
    import io
    from nele_gan_amd import dataio, inference, synth
    from nele_gan_amd import metrics as mt
    c, v = synth.batch(3, L, start=950)
    q = lambda w: (np.round(np.clip(w, -1, 1) * 32767.0) / 32768.0).astype(np.float32)
    clean_dir, enh_dir = tmp_path / 'clean', tmp_path / 'enh'
    clean_dir.mkdir()
    enh_dir.mkdir()
    names = ['a_Cafeteria.wav', 'b_Cafeteria.wav', 'c_Airport.wav']
    enh = [q(c[0] + 0.3 * v[0])[:L - 700], np.zeros(L, dtype=np.float32), q(c[2] + 0.1 * v[2])]
    files = []
    for k, n in enumerate(names):
        dataio.write_wav_pcm16(str(clean_dir / n), q(c[k]), 16000)
        files.append(str(enh_dir / n.replace('.wav', '@1.wav')))
        dataio.write_wav_pcm16(files[-1], enh[k], 16000)
    out = io.StringIO()
    res = inference.score_quality(str(clean_dir) + '/', files, groups=('Cafeteria', 'Airport'), batch=2, out=out)
    assert res['Cafeteria']['files'] == 1 and res['Airport']['files'] == 1   # the silent file has no score
    ca, _ = dataio.load(str(clean_dir / names[0]))
    ea, _ = dataio.load(files[0])
    assert len(ea) == L - 700
    one = mt.batch_hasqi(ca[:len(ea)], ea, 16000, noise='utterance', seed=0, utt_ids=[0]).cpu().numpy()[0]
    assert (res['Cafeteria']['hasqi'], res['Cafeteria']['nonlin'], res['Cafeteria']['linear']) == pytest.approx(tuple(one[:3]), rel=1e-9)
    assert res['Airport']['hasqi'] > res['Cafeteria']['hasqi']              # less noise
    text = out.getvalue()
    assert text.startswith('Cafeteria:\nHASQI is %.3f, Nonlin is %.3f, Linear is %.3f\n' % tuple(one[:3])) and 'Airport:\n' in text


def test_the_validation_all_reduce_has_one_length_on_every_rank(monkeypatch):
    """Under data parallelism a rank whose validation shard is empty joins the all-reduce of the validation sums: its vector must be as
    long as that of a rank that scored HASQI (the length follows the scorer, not the shard)."""
    import torch.distributed as tdist
    tr = _trainer()
    seen = []
    monkeypatch.setattr(tdist, 'all_reduce', lambda t, *a, **k: seen.append(t.numel()))
    tr.world = 2
    assert tr._validate(1, [], None, None) == {}                            # nothing to report from zeros, but the collective was joined
    b = _batches()[0]
    tr._validate(1, [b], None, None)
    tr.world = 1
    assert len(seen) == 2 and seen[0] == seen[1] == 2 * len(tr.metrics) + 1 + 3 + 4, seen
