"""GPU: GanTrainer(room=...) - the metric targets of a batch that brings rir_ids are taken on Room.apply's pair; everything else is
what it is without a room."""
import os
import shutil
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rir(n=3000, seed=5, peak_at=37):
    rng = np.random.default_rng(seed)
    h = rng.standard_normal(n) * np.exp(-np.arange(n) / 400.0) * 0.2
    h[peak_at] = 1.0
    return h.astype(np.float32)


def _bank():
    from nele_gan_amd import room
    return room.RirBank({'MIRD_610': _rir(), 'AIR_stairway21': _rir(1700, 6, 5)})


def _batch(B=4, L=32768, start=70):
    from nele_gan_amd import synth
    c, v = synth.batch(B, L, start=start)
    return torch.from_numpy(c).cuda(), torch.from_numpy(v).cuda()


def _weights(tr):
    tr.flush()
    return [t.clone() for t in list(tr.G.state_dict().values()) + list(tr.D.state_dict().values())]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


METRICS = 'siib&estoi'


def test_true_metrics_in_a_room_are_the_metrics_of_room_apply():
    from nele_gan_amd import metrics as mt
    from nele_gan_amd.train_nele import GanTrainer
    bank = _bank()
    tr = GanTrainer(METRICS, room=bank)
    cw, nw = _batch()
    enh = (cw * 1.5).contiguous()                                # as out of generate(): 256 * (L // 256) columns
    ids = np.asarray([0, 1, -1, 1], np.int32)
    lens = torch.tensor([32768, 30000, 32768, 25000], dtype=torch.int32).cuda()
    tgt = tr.true_metrics(cw, enh, nw, lengths=lens, rir_ids=ids)
    x, y, la = tr.room.apply(cw, enh, nw, ids, tr.enhanced_lengths(lens))
    ref = torch.stack([mt.batch_siib(x, y, lengths=la)[1], mt.batch_estoi(x, y, lengths=la)[1]], dim=1)
    assert torch.equal(tgt, ref)
    plain = tr.true_metrics(cw, enh, nw, lengths=lens)
    assert not torch.equal(plain, tgt)
    assert torch.equal(plain, GanTrainer(METRICS).true_metrics(cw, enh, nw, lengths=lens))     # without rir_ids: what a trainer without a room gives
    # the pair = two calls
    drc = (cw * 0.8).contiguous()
    pa, pb = tr.true_metrics_pair(cw, enh, drc, nw, lengths=lens, rir_ids=ids)
    assert torch.equal(pa, tgt)
    assert torch.equal(pb, tr.true_metrics(cw, drc, nw, lengths=lens, resynth=False, rir_ids=ids))
    da, db = tr.true_metrics_pair(cw, enh, drc, nw, lengths=lens, rir_ids=ids, defer=True).result()
    assert torch.equal(da, pa) and torch.equal(db, pb)
    # a padded batch = its rows scored alone
    for b in range(4):
        n = int(lens[b])
        alone = tr.true_metrics(cw[b:b + 1, :n].contiguous(), enh[b:b + 1, :256 * (n // 256)].contiguous(), nw[b:b + 1, :n].contiguous(), rir_ids=ids[b:b + 1])
        assert torch.equal(alone[0], tgt[b]), b


def test_clean_cache_keys_carry_the_rir():
    from nele_gan_amd.train_nele import GanTrainer
    bank = _bank()
    cw, nw = _batch(2)
    enh = (cw * 1.5).contiguous()
    cold = GanTrainer('siib&haspi&estoi', room=bank)
    want = {k: cold.true_metrics(cw, enh, nw, rir_ids=np.asarray(k, np.int32)) for k in ((0, 0), (1, 1), (-1, 0))}
    tr = GanTrainer('siib&haspi&estoi', room=bank)
    tr.enable_clean_cache()
    keys = ['utt_a', 'utt_b']
    for rnd in range(2):                                         # second round: every state comes from the cache
        for k in ((0, 0), (1, 1), (-1, 0), (0, 0)):              # the same utterance keys under one RIR, another, none, the first again
            got = tr.true_metrics(cw, enh, nw, rir_ids=np.asarray(k, np.int32), keys=keys)
            assert torch.equal(got, want[k]), (rnd, k)
    assert tr.clean_cache.hits > 0


def test_canonical_step_in_a_room_plain_and_pipelined():
    from nele_gan_amd.train_nele import GanTrainer
    bank = _bank()
    batches = [_batch(4, 32768, start=70 + 10 * k) for k in range(3)]
    ids = [np.asarray(v, np.int32) for v in ([0, 1, -1, 1], [1, 1, 0, 0], [-1, 0, 1, 0])]
    lens = torch.tensor([32768, 30000, 32768, 26000], dtype=torch.int32).cuda()

    def run(pipelined, early=None):
        tr = GanTrainer(METRICS, room=bank)
        tgts, pre = [], None
        for k, (cw, nw) in enumerate(batches):
            nb = (batches[k + 1][0], batches[k + 1][1], lens) if (pipelined and k + 1 < len(batches)) else None
            _, _, tgt = tr.canonical_step(cw, nw, lengths=lens, pre=pre, next_batch=nb, rir_ids=ids[k], early=early)
            pre = tr.prefetched if pipelined else None
            if not pipelined:                                   # the step's targets are true_metrics of the batch it generated
                assert torch.equal(tgt, tr.true_metrics(cw, tr._last_enh, nw, lengths=lens, rir_ids=ids[k]))
            tgts.append(tgt.clone())
        st = tr.check_status()
        assert st['skipped_g_steps'] == st['skipped_d_steps'] == 0
        return tgts, _weights(tr)
    t0, w0 = run(False)
    for early in (True, False):
        t1, w1 = run(True, early)
        assert all(torch.equal(a, b) for a, b in zip(t0, t1)) and _same(w0, w1), early


def test_room_none_changes_nothing_and_a_room_does():
    from nele_gan_amd.train_nele import GanTrainer
    bank = _bank()
    batches = [_batch(4, 32768, start=70 + 10 * k) for k in range(2)]
    ids = np.asarray([0, 1, 1, 0], np.int32)

    def run(**kw):
        tr = GanTrainer(METRICS, **{k: v for k, v in kw.items() if k != 'ids'})
        for cw, nw in batches:
            tr.canonical_step(cw, nw, **({'rir_ids': kw['ids']} if 'ids' in kw else {}))
        return _weights(tr)
    base = run()
    assert _same(base, run(room=None))
    assert _same(base, run(room=bank))                           # a room, but batches without rir_ids
    assert not _same(base, run(room=bank, ids=ids))


def test_epoch_and_fit_from_files_named_after_their_rir(tmp_path):
    """the toy triple, its files renamed to carry an RIR field, and a bank of two synthetic RIRs (seeded decaying noise)"""
    from nele_gan_amd import dataio
    from nele_gan_amd.train_nele import GanTrainer
    toy, root = os.path.join(ROOT, 'tests', 'golden', 'toy'), str(tmp_path)
    names = ['toy#MIRD_610#a.wav', 'toy#AIR_stairway21#a.wav', 'toy#none#a.wav']
    for part, kinds in (('Train', ('Clean', 'Noise', 'MultiEnh')), ('Test', ('Clean', 'Noise'))):
        for kind in kinds:
            os.makedirs(os.path.join(root, part, kind))
            for n in names:
                shutil.copy(os.path.join(toy, '%s_%s.wav' % (part, kind)), os.path.join(root, part, kind, n))
    train = sorted(dataio.get_filepaths(root + '/Train/Clean/'))
    test = sorted(dataio.get_filepaths(root + '/Test/Clean/'))
    bank = _bank()
    assert sorted(bank.ids(names).tolist()) == [-1, 0, 1]

    def epoch(room_on):
        tr = GanTrainer(METRICS, room=bank if room_on else None)
        fb = dataio.FileBatches(train, root + '/Train/Noise/', batch=3, drc_path=root + '/Train/MultiEnh/', rir_bank=bank if room_on else None)
        vb = dataio.FileBatches(test, root + '/Test/Noise/', batch=3, rir_bank=bank if room_on else None)
        try:
            assert ('rir' in fb[0]) == room_on
            res = tr.run_epoch(1, fb, vb, d_eval=True)
        finally:
            fb.close()
            vb.close()
        st = tr.check_status()
        assert not any(st[k] for k in ('siib_undefined', 'haspi_below_threshold', 'skipped_g_steps', 'skipped_d_steps'))
        return res
    with_room, without = epoch(True), epoch(False)
    assert with_room['samples'] == without['samples'] == 6
    assert with_room['target_mean'] != without['target_mean'] and with_room['valid'] != without['valid']

    tr = GanTrainer(METRICS, room=bank)
    res = tr.fit(train, root + '/Train/Noise/', test, root + '/Test/Noise/', train_enh_path=root + '/Train/MultiEnh/', epochs=2, sampling=3, valid_samples=3,
                 batch=3, output_path=root + '/out', pt_dir=root + '/chkpt', log_path=root + '/log.txt', clean_cache=True, rir_bank=bank)
    assert [r['g_steps'] for r in res] == [0, 1] and all(r['valid'] is not None and r['samples'] == 6 for r in res)
    st = tr.check_status()
    assert not any(st[k] for k in ('siib_undefined', 'haspi_below_threshold', 'skipped_g_steps', 'skipped_d_steps'))
    ck = torch.load(root + '/chkpt/chkpt_2.pt', map_location='cpu')
    assert ck['room'] == bank.record() and ck['room']['names'] == ['MIRD_610', 'AIR_stairway21']
    again = GanTrainer(METRICS, room=bank)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter('always')
        again.load_checkpoint(root + '/chkpt/chkpt_2.pt')
    assert not [w for w in seen if 'room' in str(w.message)]
    assert again.loaded_room == bank.record()
    with pytest.warns(UserWarning, match='room'):
        GanTrainer(METRICS).load_checkpoint(root + '/chkpt/chkpt_2.pt')
