"""CPU: the premises of tests/test_estoi_stages_gpu.py, from oracle/estoi.py alone.  The stage tests compare `keep` exactly and rely on
each case sitting on the edge it is named after; if a premise failed, the GPU tests could pass without testing what they claim."""
import numpy as np
import pytest

import estoi_cases as C


@pytest.mark.parametrize('name', sorted(C.EXPECTED))
def test_sizes_and_kept_counts(name):
    L, n10, F, kept = C.EXPECTED[name]
    x, y = C.case(name)
    ref = C.reference(name)
    assert len(x) == len(y) == L and x.dtype == y.dtype == np.float32
    assert C.dims(L) == (n10, F) and ref['xr'].shape == (2, n10) and len(ref['en']) == F
    assert ref['nkept'] == kept == len(ref['keep']) and ref['tob'].shape == (2, 15, kept) and len(ref['dseg']) == max(kept - 29, 0)


def test_block_tail_lengths_sit_on_the_resampler_block():
    assert C.EXPECTED['tail_2048'][1] == 1280 and C.EXPECTED['tail_2049'][1] == 1281       # five outputs per thread, 256 threads
    assert C.EXPECTED['one_frame_409'][1:3] == (256, 1) and C.EXPECTED['one_frame_410'][1:3] == (257, 1)
    assert len(C.ragged()[3][5][0]) == 100 < 117                                            # shorter than one phase of the filter


def test_no_frame_lies_near_the_gate():
    """keep / nkept are compared exactly: that is only fair when float64 rounding cannot move a frame across max - 40 dB."""
    margins = {name: C.reference(name)['margin'] for name in C.EXPECTED}
    margins.update({'ragged[%d]' % b: r['margin'] for b, r in enumerate(C.ragged_reference())})
    print(margins)
    assert min(margins.values()) > C.GATE_MARGIN_DB
    assert 0.05 < margins['gapped_64000'] < 0.2                                             # the tightest case: 0.10 dB
    for name in ('frames29_6347', 'frames30_6348', 'frames30_6349'):                      # stationary noise: every frame far inside
        assert margins[name] > 30.0


def test_29_frames_score_the_constant_and_30_a_real_score():
    assert C.reference('frames29_6347')['raw'] == 1e-5
    for name in ('frames30_6348', 'frames30_6349'):
        ref = C.reference(name)
        assert len(ref['dseg']) == 1 and 0.2 < ref['raw'] < 0.8 and ref['raw'] == pytest.approx(ref['dseg'][0], rel=1e-12)
    for name in ('tail_2048', 'tail_2049', 'one_frame_409', 'one_frame_410'):
        assert C.reference(name)['raw'] == 1e-5


def test_gapped_case_keeps_frame_256_at_a_shifted_position():
    ref = C.reference('gapped_64000')
    keep = ref['keep']
    assert np.count_nonzero(np.diff(keep) > 1) >= 3                                       # not contiguous
    assert keep[142] == 256 and keep[141] < 256                                           # second scan chunk starts mid-list
    assert 0.2 < ref['raw'] < 0.35 and len(ref['dseg']) == 151
    assert ref['raw'] == pytest.approx(np.mean(ref['dseg']), rel=1e-12)


def test_ragged_batch_layout():
    X, Y, lengths, rows = C.ragged()
    refs = C.ragged_reference()
    assert X.shape == Y.shape == (7, C.RAGGED_L) and list(lengths) == [6349, 6347, 2049, 6349, 409, 100, 0]
    for b, n in enumerate(lengths):
        assert np.isnan(X[b, n:]).all() and np.isnan(Y[b, n:]).all() and np.isfinite(X[b, :n]).all() and np.isfinite(Y[b, :n]).all()
    assert not X[3].any() and not Y[3].any()                                              # digital silence, full length
    assert np.isnan(refs[3]['raw']) and refs[3]['nkept'] == 30 and np.isnan(refs[3]['dseg']).all() and not refs[3]['tob'].any()
    assert [r['nkept'] for r in refs] == [30, 29, 9, 30, 1, 0, 0]
    assert [r['raw'] for r in refs[4:]] == [1e-5] * 3 and refs[1]['raw'] == refs[2]['raw'] == 1e-5 and 0.2 < refs[0]['raw'] < 0.8
