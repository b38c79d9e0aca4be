"""GPU: SIIB's lag products on the float64 matrix cores (csrc/siib.hip, siib_lag_kernel).

The 28 x 28 x (15 or 29) lag products of the band rows are one MFMA product per frame segment: M = the bands of a, N = (lag, band of b),
K = frames, LDS chunks of 32 frames.  What can go wrong there sits at the chunk and segment ends (a segment length is no multiple of the
chunk or of the 4-frame k-step), at utterances shorter than one chunk, in the padding rows and columns of the last tiles, and in who
computes a segment (the batch-size classes): the cases below.  The reference is the projection path of the test library
(NELE_SIIB_LAG=0: 420 x 420 x n products over the stacked frames), which shares nothing with the lag kernels."""
import os
import subprocess
import sys

import numpy as np
import pytest
from conftest import ab_env

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
HERE = os.path.dirname(__file__)

# the batch lives in the plain case module (the stage tests' CPU premises use it too)
from siib_cases import RAGGED_LENS as LENS, SPARSE, ragged_batch  # noqa: E402,F401


_CHILD = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
from nele_gan_amd import metrics as mt
import test_siib_lag_mfma_gpu as T
c, y = T.ragged_batch()
raw, _, info = mt.batch_siib(c, y, lengths=torch.tensor(T.LENS, dtype=torch.int32), return_info=True)
np.save(sys.argv[2], np.concatenate([raw.double().cpu().numpy(), info.cpu().numpy().astype(np.float64).ravel()]))
'''


def test_lag_mfma_against_the_projection_path(tmp_path):
    """Default (lag products on MFMA) against NELE_SIIB_LAG=0 in the test library, separate processes (the switch is read once).  Same
    mathematics in another summation order: the float32 scores are at most a couple of ulps apart (rtol 3e-7, the tolerance of
    test_siib_lag_products_equal_the_stacked_frame_gemms); M, frame counts and status are equal."""
    res = []
    for flag in ('1', '0'):
        out = str(tmp_path / ('lag_%s.npy' % flag))
        subprocess.run([sys.executable, '-c', _CHILD, os.path.dirname(HERE), out], check=True, env=ab_env(NELE_SIIB_LAG=flag), timeout=240)
        res.append(np.load(out))
    B = len(LENS)
    raw, info = res[0][:B], res[0][B:].reshape(B, 4).astype(np.int64)
    print('raw lag', raw, 'raw projection', res[1][:B], 'active frames', info[:, 2])
    na = info[:, 2]
    assert info[:, 3].tolist() == [0, 0, 1, 1, 0], info  # bit 1: replication factor capped at 40 (the 9 600-sample and the sparse utterance)
    assert 16 <= na[SPARSE] < 58, na                     # the sparse utterance: less than one chunk of the old kernel
    assert (na % 4 != 0).any(), na                       # a segment that ends inside a k-step
    assert np.all(np.isfinite(raw))
    np.testing.assert_array_equal(res[0][B:], res[1][B:])
    np.testing.assert_allclose(raw, res[1][:B], rtol=3e-7, atol=0)


def test_utterance_with_too_few_active_frames():
    """ncols = active frames - 14 < 2.  The replication rule tiles any utterance to 25 s of active speech or 40 times, so only an
    utterance of a few samples gets there: 60 samples, 40 copies, 10 frames.  The lag kernels still run over the frames there are (less
    than one chunk, three empty segments), siib_assemble_kernel writes zero matrices, and the score is NaN with status bits 1 (M capped)
    and 8 - and the utterance beside it is scored as if it were alone."""
    from nele_gan_amd import metrics as mt, synth
    c, v = synth.batch(2, 64000, start=320)
    y = (0.8 * c + v).astype(np.float32)
    p = int(np.argmax(np.abs(c[0])))
    c[0, :60], y[0, :60] = c[0, p:p + 60].copy(), y[0, p:p + 60].copy()
    raw, _, info = mt.batch_siib(c, y, lengths=[60, 64000], return_info=True)
    raw, info = raw.cpu().numpy(), info.cpu().numpy()
    print('raw', raw, 'info', info)
    assert info[0, 2] - 14 < 2, info
    assert info[0, 3] == 9 and np.isnan(raw[0])
    assert info[1, 3] == 0 and np.isfinite(raw[1])
    solo, _ = mt.batch_siib(c[1:], y[1:])
    assert raw[1:].tobytes() == solo.cpu().numpy().tobytes()


def test_score_is_bit_identical_alone_and_in_a_batch_of_three():
    """A segment is summed from zero in frame order whichever workgroup gets it (four segments per workgroup group at B = 3 as at B = 1, but
    other rows beside it): the raw float32 score of an utterance is the same alone, in row 0 and in the last row."""
    from nele_gan_amd import metrics as mt, synth
    c, v = synth.batch(3, 63871, start=330)
    y = (0.8 * c + v).astype(np.float32)
    solo = mt.batch_siib(c[:1], y[:1])[0].cpu().numpy()
    raw3 = mt.batch_siib(c, y)[0].cpu().numpy()
    last = mt.batch_siib(c[::-1].copy(), y[::-1].copy())[0].cpu().numpy()
    assert np.isfinite(solo).all()
    assert solo.tobytes() == raw3[:1].tobytes() == last[2:].tobytes()
