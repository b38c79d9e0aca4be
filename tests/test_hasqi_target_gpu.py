"""GPU: HASQI v2 (pyhaspi2.py:32-74) as a batched training target - nele_metric_hasqi_var through metrics.batch_hasqi / HasqiSplit:
parity with the reference's golden run and the noise-free oracle (the tolerances of tests/test_haspi_quality_gpu.py), equality with
the one-shot HASPI-v1 + HASQI call, the clean / degraded split, per-utterance lengths, batch invariance of the per-utterance noise,
the clean-state sections, hearing loss and undefined input."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
Q = np.load(os.path.join(GOLD, 'haspi_quality.npz'))
RTOL = 2e-5
# columns of batch_haspi_quality that batch_hasqi's seven are: Combined, Nonlin, Linear, CepCorr, BMsync5, Dloud, Dslope
ONE_SHOT = [5, 6, 7, 1, 8, 9, 10]
_memo = {}


def _batch16():
    """Three 1 s utterances at 16 kHz with more and more noise (shared, read-only)."""
    if 'b16' not in _memo:
        from nele_gan_amd import synth
        c, v = synth.batch(3, 16000, start=4100)
        y = (c + np.array([0.2, 0.6, 1.5], dtype=np.float32)[:, None] * v).astype(np.float32)
        _memo['b16'] = (torch.from_numpy(c).cuda(), torch.from_numpy(y).cuda())
    return _memo['b16']


def _eq(a, b):
    np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())


def test_golden_pair_matches_the_reference_and_the_noise_free_oracle():
    from nele_gan_amd import metrics as mt
    from oracle import haspi as H
    x, y = Q['x'], Q['y']
    out, info = mt.batch_hasqi(x, y, 24000, noise=False, return_info=True)
    o = out[0].cpu().numpy()
    assert out.shape == (1, 7) and out.dtype == torch.float64
    assert int(info[0, 1]) == 0 and int(info[0, 0]) > 100 and int(info[0, 2]) > 100
    q = H.hasqi_v2(x, 24000, y, 24000)
    print('hasqi', o.tolist(), 'oracle', q)
    np.testing.assert_allclose(o[:3], [q[0], q[1], q[2]], rtol=RTOL)
    np.testing.assert_allclose(o[4:7], [q[3][1], q[3][2], q[3][3]], rtol=RTOL)
    np.testing.assert_allclose(o[:3], Q['hasqi'], atol=1e-3)                # the reference's own (noisy) run


def test_all_seven_values_equal_the_one_shot_call():
    from nele_gan_amd import metrics as mt
    c, y = _batch16()
    got = mt.batch_hasqi(c, y, 16000, noise=False).cpu().numpy()
    one = mt.batch_haspi_quality(c, y, 16000, noise=False).cpu().numpy()
    np.testing.assert_allclose(got, one[:, ONE_SHOT], rtol=1e-9)
    assert np.all(np.diff(got[:, 0]) < 0)                                   # more noise, lower quality
    assert mt.QUALITY_TARGET_FIELDS == ('Nonlin', 'Linear') and mt.HASQI_FIELDS[1:3] == mt.QUALITY_TARGET_FIELDS


@pytest.mark.parametrize('noise', [False, 'utterance'])
def test_split_is_bit_identical_to_phase_0(noise):
    from nele_gan_amd import metrics as mt
    c, y = _batch16()
    y2 = (c + 0.3 * (y - c)).contiguous()
    ids = torch.tensor([7, 8, 9])
    kw = dict(noise=noise, seed=3, utt_ids=ids)
    a, a2 = mt.batch_hasqi(c, y, 16000, **kw), mt.batch_hasqi(c, y2, 16000, **kw)
    sp = mt.HasqiSplit(c, fs=16000, **kw)
    assert sp.clean_part() is False
    b = sp.degraded_part(y)
    b2 = sp.degraded_part(y2)                                               # a second processed version on the same clean half
    _eq(a, b)
    _eq(a2, b2)
    assert not np.array_equal(a.cpu().numpy(), a2.cpu().numpy())


def test_mixed_lengths_in_one_padded_batch_equal_the_per_file_calls():
    from nele_gan_amd import dataio
    from nele_gan_amd import metrics as mt
    from nele_gan_amd import synth
    c, v = synth.batch(3, 24000, start=4200)
    lens = [24000, 17000, 20480]
    xs = [c[b, :n] for b, n in enumerate(lens)]
    ys = [(c[b, :n] + 0.5 * v[b, :n]).astype(np.float32) for b, n in enumerate(lens)]
    xp, L = dataio.pad_batch(xs)
    yp, _ = dataio.pad_batch(ys)
    xp[2, lens[2]:] = -3.0                                                  # garbage behind a row's end must not matter
    yp[1, lens[1]:] = 7.0
    got = mt.batch_hasqi(xp, yp, 16000, lengths=torch.from_numpy(L), noise=False).cpu().numpy()
    for b in range(3):
        one = mt.batch_hasqi(xs[b], ys[b], 16000, noise=False).cpu().numpy()[0]
        np.testing.assert_allclose(got[b], one, rtol=1e-9, err_msg=str(b))


def test_per_utterance_noise_is_batch_invariant_and_row_keyed_noise_is_not():
    from nele_gan_amd import metrics as mt
    c, y = _batch16()
    c5, y5 = torch.cat([c, c[:2]]), torch.cat([y, y[:2]])
    ids5 = torch.tensor([40, 41, 42, 43, 44])
    quiet = mt.batch_hasqi(c[:1], y[:1], 16000, noise=False)[0]

    def three_ways(noise):
        kw = dict(noise=noise, seed=21)
        alone = mt.batch_hasqi(c[:1], y[:1], 16000, utt_ids=ids5[:1], **kw)[0]
        row0 = mt.batch_hasqi(c, y, 16000, utt_ids=ids5[:3], **kw)[0]
        perm = [4, 2, 0, 1, 3]                                              # utterance 0 (id 40) at row 2 of 5
        row2 = mt.batch_hasqi(c5[perm].contiguous(), y5[perm].contiguous(), 16000, utt_ids=ids5[perm], **kw)[2]
        return alone, row0, row2
    alone, row0, row2 = three_ways('utterance')
    _eq(alone, row0)
    _eq(alone, row2)
    assert not np.array_equal(alone.cpu().numpy(), quiet.cpu().numpy())     # the noise is there
    np.testing.assert_allclose(alone.cpu().numpy(), quiet.cpu().numpy(), atol=2e-3)
    other = mt.batch_hasqi(c[:1], y[:1], 16000, noise='utterance', seed=21, utt_ids=torch.tensor([41]))[0]
    assert not np.array_equal(alone.cpu().numpy(), other.cpu().numpy())     # and it is the utterance's own
    alone, row0, row2 = three_ways(True)
    _eq(alone, row0)                                                        # row 0 either way
    assert not np.array_equal(alone.cpu().numpy(), row2.cpu().numpy())      # keyed by the row: the position shows


def test_phase_4_on_the_named_sections_alone():
    """The bytes nele_metric_hasqi_clean_sections names, copied into a workspace of 0xFF bytes at other rows of a batch of another
    size, are all phase 4 needs."""
    from nele_gan_amd import _lib
    from nele_gan_amd import metrics as mt
    c, y = _batch16()
    ids = torch.tensor([5, 6, 7])
    L, fs = c.shape[1], 16000
    sp = mt.HasqiSplit(c, fs=fs, noise='utterance', seed=9, utt_ids=ids)
    sp.clean_part()
    ref = sp.degraded_part(y)

    def sections(B):
        buf = (ctypes.c_longlong * 72)()
        n = _lib.lib.nele_metric_hasqi_clean_sections(B, L, fs, buf, 24)
        assert 0 < n <= 24
        return [(int(buf[3 * k]), int(buf[3 * k + 1]), int(buf[3 * k + 2])) for k in range(n)]
    rows = [2, 0]
    sp2 = mt.HasqiSplit(torch.zeros_like(c[rows]), fs=fs, noise='utterance', seed=9, utt_ids=ids[rows], ws_kind='hasqi_sections_test')
    sp2.ws.fill_(255)
    for (o3, st3, nb), (o2, st2, nb2) in zip(sections(3), sections(2)):
        assert nb == nb2
        if st3 == 0:
            sp2.ws[o2:o2 + nb].copy_(sp.ws[o3:o3 + nb])
            continue
        for k, r in enumerate(rows):
            sp2.ws[o2 + k * st2:o2 + k * st2 + nb].copy_(sp.ws[o3 + r * st3:o3 + r * st3 + nb])
    got = sp2.degraded_part(y[rows].contiguous())
    _eq(got, ref[rows])
    per_utt = sum(nb for (_o, st, nb) in sections(1) if st > 0)
    assert per_utt < 24000 * 32 * 4 * 1.05                                  # the BM motion of x and little else: no per-sample envelope


def test_hearing_loss_matches_the_oracle():
    sys.path.insert(0, GOLD)
    from make_golden_haspi import HL_MILD
    from nele_gan_amd import metrics as mt
    from oracle import haspi as H
    G = np.load(os.path.join(GOLD, 'haspi_hl.npz'))
    x, y = G['x'], G['y']
    o = mt.batch_hasqi(x, y, 24000, noise=False, HL=HL_MILD).cpu().numpy()[0]
    q = H.hasqi_v2(x, 24000, y, 24000, HL=HL_MILD)
    print('hasqi HL', o.tolist(), 'oracle', q)
    np.testing.assert_allclose(o[[0, 1, 2, 4, 5, 6]], [q[0], q[1], q[2], q[3][1], q[3][2], q[3][3]], rtol=2e-5, atol=2e-6)
    normal = mt.batch_hasqi(x, y, 24000, noise=False).cpu().numpy()[0]
    assert abs(o[0] - normal[0]) > 1e-3                                     # the loss really changes the score


def test_a_silent_row_is_flagged_and_the_others_are_unaffected():
    from nele_gan_amd import metrics as mt
    c, y = _batch16()
    good = mt.batch_hasqi(c, y, 16000, noise=False)
    ys = y.clone()
    ys[1] = 0.0
    out, info = mt.batch_hasqi(c, ys, 16000, noise=False, return_info=True)
    assert int(info[1, 1]) & 1 and bool(torch.isnan(out[1]).all())
    assert int(info[0, 1]) == 0 and int(info[2, 1]) == 0
    _eq(out[[0, 2]], good[[0, 2]])
