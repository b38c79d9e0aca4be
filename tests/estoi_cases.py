"""Inputs and float64 references of the ESTOI stage tests (tests/test_estoi_stages_gpu.py on the device, tests/test_estoi_cases_cpu.py for
the premises).  Plain module: numpy and oracle/estoi.py only, nothing here touches a GPU.

A case is a pair (x clean, y degraded) of float32 signals at 16 kHz, chosen to sit on an edge of csrc/estoi.hip:
  tail_2048 / tail_2049      n10 = 1280 / 1281: exactly one block of estoi_resample5_kernel / a second block that holds ONE output
  one_frame_409 / _410       n10 = 256 / 257: a single frame (F = 1), score 1e-5
  frames29_6347              29 frames, all kept: the last length that scores the constant 1e-5
  frames30_6348 / _6349      30 frames, all kept: ONE segment (estoi_final_kernel with J = 1), a real score
  gapped_64000               311 frames of which 180 are kept, in four runs: the kept frames are not contiguous and original frame 256
                             (the second 256-frame chunk of the compaction scan of estoi_vad_kernel) lands at kept position 142
and ragged(): one padded batch that mixes them with rows that have no frame at all and a digital-silence row."""
import functools

import numpy as np

from oracle import estoi as E

GATE_MARGIN_DB = 1e-6           # no frame of any case may lie this close to the gate max - 40 dB (seven orders above float64 rounding)
# name -> (L, n10, F, kept frames)
EXPECTED = {
    'tail_2048': (2048, 1280, 9, 9),
    'tail_2049': (2049, 1281, 9, 9),
    'one_frame_409': (409, 256, 1, 1),
    'one_frame_410': (410, 257, 1, 1),
    'frames29_6347': (6347, 3967, 29, 29),
    'frames30_6348': (6348, 3968, 30, 30),
    'frames30_6349': (6349, 3969, 30, 30),
    'gapped_64000': (64000, 40000, 311, 180),
}
GAPS = ((8000, 14000), (30000, 31000), (52000, 52600))      # samples of the gapped case's clean signal scaled by 1e-4
RAGGED_L = 6349


def dims(L):
    """-> (n10, F): samples at 10 kHz and frames of 256 at hop 128 of an L-sample signal"""
    n10 = -(-5 * L // 8)
    return n10, ((n10 - E.N_FRAME) // (E.N_FRAME // 2) + 1 if n10 >= E.N_FRAME else 0)


def noise_pair(L, seed):
    """Stationary white noise (no gaps: every frame is kept) and the same plus as much independent noise."""
    rng = np.random.default_rng(seed)
    x = 0.03 * rng.standard_normal(L)
    y = x + 0.03 * rng.standard_normal(L)
    return x.astype(np.float32), y.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    L = EXPECTED[name][0]
    if name == 'gapped_64000':
        from nele_gan_amd import synth
        c, v = synth.batch(4, L, start=40)
        x = c[1].copy()
        for a, b in GAPS:
            x[a:b] *= np.float32(1e-4)
        x, y = x, x + v[1]
    else:
        x, y = noise_pair(L, 1000 + L)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def oracle_stages(x, y):
    """Every stage of oracle/estoi.py on one row (float64): xr [2, n10], en [F], keep [nkept] (original frame indices), nkept,
    tob [2, 15, nkept], dseg [max(nkept - 29, 0)], raw (float: NaN for digital silence, as oracle.estoi.estoi) and margin = the smallest
    distance in dB of any frame from the gate (inf without frames).  A row too short for one frame has empty stages and the constant."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n10, F = dims(len(x))
    if len(x):
        xr = np.stack([E.resample_16k_to_10k(x), E.resample_16k_to_10k(y)])
    else:
        xr = np.zeros((2, 0))
    assert xr.shape == (2, n10)
    if F == 0:
        return dict(xr=xr, en=np.zeros(0), keep=np.zeros(0, dtype=np.int64), nkept=0, tob=np.zeros((2, E.NUMBAND, 0)), dseg=np.zeros(0),
                    raw=1e-5, margin=np.inf)
    w = E.hann_sym(E.N_FRAME)
    st = E.frame_starts(n10)
    en = 20 * np.log10(np.linalg.norm(w * xr[0][st[:, None] + np.arange(E.N_FRAME)[None, :]], axis=1) + E.EPS)
    xs, ys, mask = E.remove_silent_frames(xr[0], xr[1])
    assert len(en) == F == len(mask) and np.array_equal(mask, (np.max(en) - E.DYN_RANGE - en) < 0)
    obm, _ = E.thirdoct()
    tob = np.stack([np.sqrt(obm @ np.square(np.abs(E.stft(s).T))) for s in (xs, ys)])
    nk = int(mask.sum())
    assert tob.shape == (2, E.NUMBAND, nk)
    with np.errstate(invalid='ignore', divide='ignore'):
        J = max(nk - E.N + 1, 0)
        dseg = np.zeros(J)
        for m in range(J):
            dseg[m] = np.sum(E.row_col_normalize(tob[0][None, :, m:m + E.N]) * E.row_col_normalize(tob[1][None, :, m:m + E.N])) / E.N
        raw = E.estoi(x, y)
    return dict(xr=xr, en=en, keep=np.nonzero(mask)[0], nkept=nk, tob=tob, dseg=dseg, raw=raw,
                margin=float(np.min(np.abs(np.max(en) - E.DYN_RANGE - en))))


@functools.lru_cache(maxsize=None)
def reference(name):
    return oracle_stages(*case(name))


@functools.lru_cache(maxsize=None)
def ragged():
    """-> (X [7, 6349], Y, lengths, rows): one padded batch; rows[b] = (x, y) cut to the row's own length.  Both X and Y hold NaN behind each
    row's end.  Row 3 is digital silence at full length; rows 5 and 6 (100 and 0 samples) have no frame."""
    rows = [case('frames30_6349'), case('frames29_6347'), case('tail_2049'),
            (np.zeros(RAGGED_L, dtype=np.float32), np.zeros(RAGGED_L, dtype=np.float32)),
            case('one_frame_409'), noise_pair(100, 7), noise_pair(0, 8)]
    lengths = np.array([len(r[0]) for r in rows], dtype=np.int32)
    assert list(lengths) == [6349, 6347, 2049, 6349, 409, 100, 0]
    X = np.full((len(rows), RAGGED_L), np.nan, dtype=np.float32)
    Y = X.copy()
    for b, (x, y) in enumerate(rows):
        X[b, :len(x)], Y[b, :len(y)] = x, y
    for a in (X, Y, lengths):
        a.setflags(write=False)
    return X, Y, lengths, rows


@functools.lru_cache(maxsize=None)
def ragged_reference():
    return [oracle_stages(x, y) for (x, y) in ragged()[3]]
