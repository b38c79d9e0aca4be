"""CPU: what NoiseMixer draws for an utterance (pool recording, offset, SNR) is a function of (seed, utterance key, epoch) alone - not of
the batch, its size, the position in it or the rank that holds it - and the host restatement of the mixing gain."""
import numpy as np
import pytest

import p56_ref


def _mixer(seed=0, **kw):
    from nele_gan_amd.mixing import NoiseMixer
    rs = np.random.RandomState(1)
    pool = rs.randn(5, 9000).astype(np.float32)
    return NoiseMixer((pool, np.array([9000, 7001, 4000, 8999, 123], dtype=np.int32)), seed=seed, device='cpu', **kw)


KEYS = ['utt_%03d.wav' % k for k in range(40)]


def _as_dict(keys, drawn):
    return {k: (int(r), int(o), float(s)) for k, r, o, s in zip(keys, *drawn)}


def test_draw_depends_on_seed_key_and_epoch_only():
    m = _mixer()
    whole = _as_dict(KEYS, m.draw(KEYS, 3))
    perm = [KEYS[i] for i in np.random.RandomState(0).permutation(len(KEYS))]
    assert _as_dict(perm, m.draw(perm, 3)) == whole                                      # permuted
    pieces = {}
    for k0 in range(0, len(KEYS), 7):                                                     # re-batched
        pieces.update(_as_dict(KEYS[k0:k0 + 7], m.draw(KEYS[k0:k0 + 7], 3)))
    assert pieces == whole
    for rank in range(4):                                                                 # sharded over 4 ranks, each with a mixer of its own
        shard = KEYS[rank::4]
        got = _as_dict(shard, _mixer().draw(shard, 3, lengths=[100] * len(shard)))
        assert all(whole[k] == v for k, v in got.items())
    assert _as_dict(KEYS, _mixer().draw(KEYS, 3)) == whole                                # a re-run


def test_epochs_and_seeds_differ_and_draws_are_in_range():
    m = _mixer()
    a, b = m.draw(KEYS, 1), m.draw(KEYS, 2)
    assert any((x != y).any() for x, y in zip(a, b))
    assert sum(int(x != y) for x, y in zip(a[1], b[1])) > len(KEYS) // 2
    c = _mixer(seed=1).draw(KEYS, 1)
    assert (a[1] != c[1]).sum() > len(KEYS) // 2
    from nele_gan_amd import synth
    for rows, offs, snr in (a, b, c):
        assert rows.dtype == np.int32 and offs.dtype == np.int32 and snr.dtype == np.float64
        assert ((rows >= 0) & (rows < 5)).all() and (offs >= 0).all() and (offs < m.pool_lengths_host[rows]).all()
        assert set(snr.tolist()) <= set(float(s) for s in synth.SNRS_DB)
    many = _mixer().draw(['k%d' % i for i in range(600)], 0)
    assert set(many[0].tolist()) == set(range(5)) and set(many[2].tolist()) == set(float(s) for s in synth.SNRS_DB)
    assert set(_mixer(snrs_db=(0, 5)).draw(KEYS, 0)[2].tolist()) == {0.0, 5.0}


def test_bad_arguments():
    from nele_gan_amd.mixing import NoiseMixer
    with pytest.raises(ValueError):
        _mixer(level='peak')
    with pytest.raises(ValueError):
        NoiseMixer((np.zeros((2, 10), dtype=np.float32), np.array([10, 11])), device='cpu')
    with pytest.raises(ValueError):
        _mixer(snrs_db=())


def test_host_gain_restatement():
    rs = np.random.RandomState(2)
    row = rs.randn(1000)
    seg = p56_ref.mix_segment(row, 700, 650, 1500)
    assert (seg[:50] == row[650:700]).all() and (seg[50:750] == row[:700]).all() and (seg[750:1450] == row[:700]).all()
    g = p56_ref.mix_gain(seg, -5.0, 1e-3)
    assert abs(10 * np.log10(1e-3 / np.mean((g * seg) ** 2)) + 5.0) < 1e-12
    assert p56_ref.mix_gain(np.zeros(10), 0.0, 1.0) == 0.0 and p56_ref.mix_gain(seg, 0.0, 0.0) == 0.0
