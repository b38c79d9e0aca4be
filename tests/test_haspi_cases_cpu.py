"""CPU: the premises of tests/test_haspi_stages_gpu.py, from oracle/haspi.py alone.  The stage tests compare n_active, the active index
list and every compacted stage exactly and rely on each case crossing the seam it is named after; if a premise failed, the GPU tests
could pass without testing what they claim.  The chunk counts are recomputed from the constants of csrc/haspi.hip restated in
haspi_cases.py: when one of them changes there, the assertion that fails here names the case that needs another size."""
import os
import re
import sys

import numpy as np
import pytest

import haspi_cases as C

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))

GATE_MARGIN_DB = max(100 * C.LP_DB, 1e-3)         # 100 x the bound on the kernel's lp error (1.24e-2 dB), and no less than 1e-3 dB


def chunks(n, size):
    return -(-n // size)


def test_constants_are_those_of_the_kernel_file():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'nele_gan_amd', 'csrc', 'haspi.hip')).read()
    for name in ('GS_LC', 'GS_RC', 'ME_N', 'GL_N', 'RS_CH', 'CP_F', 'MS_TC', 'MS_R', 'HP_SPACE'):
        m = re.search(r'^#define %s (\d+)' % name, src, re.M)
        assert m and int(m.group(1)) == getattr(C, name), name
    assert int(re.search(r'^#define HP_MAXFIR (\d+)', src, re.M).group(1)) + 1 == C.MAXFIR


@pytest.mark.parametrize('name', sorted(C.EXPECTED))
def test_sizes_counts_and_scores(name):
    fs, L, n24, nsub, na, smin, smax, clamped = C.EXPECTED[name]
    x, y, cfs, _HL, dither = C.case(name)
    ref = C.reference(name)
    assert len(x) == len(y) == L and x.dtype == y.dtype == np.float32 and cfs == fs
    assert C.dims(L, fs) == (n24, nsub)
    assert ref['r24'].shape == ref['mid'].shape == (2, n24) and ref['env'].shape == ref['ctl'].shape == (2, n24, 32)
    assert ref['lp'].shape == (2, nsub, 32) and ref['gate'].shape == (nsub,)
    assert ref['n_active'] == na == len(ref['index']) and na > 1
    assert ref['cep'].shape == (2, 6, na) and ref['xf'].shape == (na, 50) and ref['cm'].shape == (5, 10)
    assert (int(ref['shift'].min()), int(ref['shift'].max())) == (smin, smax)
    assert int(np.sum(ref['bw'][0] == ref['bwmin'][0])) == clamped
    assert np.isfinite(ref['raw']) and 1.0 < ref['raw'] < float(np.sum(C.H.WEIGHTS))
    assert dither is None or dither.shape == (2, nsub, 32)


def test_the_restated_chain_is_haspi_v2():
    """haspi_cases.oracle_stages restates haspi_v2's chain (so that it can also start behind the resampler): same score, bit for bit."""
    for name in sorted(C.EXPECTED):
        x, y, fs, HL, dither = C.case(name)
        ref = C.reference(name)
        dx, dy = (None, None) if dither is None else (dither[0, :ref['n_active']], dither[1, :ref['n_active']])
        raw, parts = C.H.haspi_v2(x, fs, y, fs, dither_x=dx, dither_y=dy, return_parts=True, HL=HL)
        assert raw == ref['raw'] and np.array_equal(parts['index'], ref['index']) and np.array_equal(parts['CM'][1:6], ref['cm'])
        assert np.array_equal(parts['xsl'].T, ref['env'][0]) and np.array_equal(parts['ymid'], ref['mid'][1])
        assert np.array_equal(np.asarray(parts['x24'], dtype=np.float32), ref['r24'][0]) and parts['xdB'].shape == parts['xsl'].shape
        assert np.array_equal(parts['Xmod'][3][7], ref['xf'][:, 27])
        # started from its own r24, the chain gives the same stages
        again = C.oracle_stages(x, y, fs, HL=HL, dither=dither, r24=ref['r24'])
        assert again['raw'] == ref['raw'] and np.array_equal(again['lp'], ref['lp'])


def test_the_asserted_bounds_stay_inside_their_budgets():
    """The constants of test_haspi_stages_gpu.py against the a-priori budgets they must not exceed."""
    T = pytest.importorskip('test_haspi_stages_gpu')
    assert 5.5e-5 < T.ENV_DB < 6.5e-5 and 1.2e-4 < T.LP_DB < 1.3e-4 and T.LP_DB == C.LP_DB
    assert T.CEP_DB <= T.CEP_DB_PRIORI and T.XF_DB <= T.XF_DB_PRIORI and T.BW_ABS <= T.bw_budget() < 1e-8
    assert T.R24_REL_24K <= 16 * T.U32 and T.R24_REL_RS <= 4e-5 and T.CTL_REL < 1.01 * T.U32
    assert T.SUMW * T.CM_ABS + T.U32 * 10 < 4e-5                                          # raw: far below the 1e-4 relative of the score-level tests


def test_no_frame_lies_near_the_silence_gate():
    """n_active, index and every compacted stage are compared exactly: fair only when the kernel's lp error (bounded by LP_DB, a hundredth
    of this margin at most) cannot move a frame across 2.5 dB."""
    margins = {name: C.reference(name)['margin'] for name in C.EXPECTED}
    margins.update({'ragged[%d]' % b: r['margin'] for b, r in enumerate(C.ragged_reference())})
    print(margins)
    assert min(margins.values()) > GATE_MARGIN_DB
    assert min(margins.values()) > 0.05                                                   # the tightest: zeros_11987, 0.0595 dB


def test_every_case_crosses_its_seam():
    E = C.EXPECTED
    # the minimum: the fewest chunks any call can have (two scan and middle-ear chunks, one of everything else), fewer frames than the
    # longest modulation FIR has taps, and channels whose first frames' windows end before the shifted envelope starts (shift > 26 + 9)
    n24, nsub, na = E['min_2400'][2:5]
    assert chunks(n24, C.GS_LC) == 2 and chunks(n24, C.ME_N) == 2 and chunks(nsub, C.MS_TC) == 1
    assert na < nsub < C.MAXFIR < C.MS_R and E['min_2400'][6] > 26 + 9
    # zeros: many chunks of every kind, no multiple of any group size, two modulation chunks of ACTIVE frames, a gap in the kept frames
    n24, nsub, na = E['zeros_11987'][2:5]
    assert n24 % 9 and n24 % C.GS_RC and n24 % 32
    assert chunks(n24, C.GS_LC) == 8 and chunks(n24, C.ME_N) == 6 and chunks(n24, C.GL_N) == 6 and chunks(nsub, C.CP_F) == 11
    assert chunks(na, C.MS_TC) == 2 and nsub > na > C.MS_TC
    ref = C.reference('zeros_11987')
    x, y = C.case('zeros_11987')[:2]
    assert not x[:C.ZERO_HEAD].any() and not y[:C.ZERO_HEAD].any() and not x[C.ZERO_GAP[0]:C.ZERO_GAP[1]].any() and y[C.ZERO_GAP[0]:C.ZERO_GAP[1]].any()
    assert not ref['ctl'][:, :C.ZERO_HEAD].any() and not ref['env'][:, :C.ZERO_HEAD].any()   # |u|^2 = 0 exactly: log2(0), the 1e-30 clip
    gaps = np.nonzero(np.diff(ref['index']) > 1)[0]
    assert len(gaps) == 1 and ref['index'][gaps[0] + 1] - ref['index'][gaps[0]] > C.CP_F     # a whole gate block without a kept frame
    # the three seam cases: two chunks that end on the row's end, and a third chunk that holds one sample / one 16-sample group
    assert E['seam_3072'][2] == 2 * C.GS_LC and E['seam_3071'][2] == 2 * C.GS_LC - 1 and E['seam_3073'][2] == 2 * C.GS_LC + 1
    assert [chunks(E[k][2], C.GS_LC) for k in ('seam_3071', 'seam_3072', 'seam_3073')] == [2, 2, 3]
    # the resamplers
    fs, L, n24 = E['rs16k_9001'][:3]
    assert fs == 16000 and L % 2 == 1 and int(L * 1.5) == n24 - 1 and chunks(n24, C.RS_CH) == 18     # resampy writes n24 - 1 outputs
    assert C.reference('rs16k_9001')['r24'][:, -1].tolist() == [0.0, 0.0] and C.reference('rs16k_9001')['r24'][:, -2].all()
    assert E['rs22k_10000'][0] == 22050 and chunks(E['rs22k_10000'][2], C.RS_CH) == 15
    assert E['rs8k_5000'][0] == 8000 and E['rs8k_5000'][2] == 3 * E['rs8k_5000'][1] and chunks(E['rs8k_5000'][2], C.RS_CH) == 20
    # band-limited: clamped channels beside interpolated ones, and high channels near 0 dB
    ref = C.reference('lowband_6000')
    cl = ref['bw'][0] == ref['bwmin'][0]
    assert int(cl.sum()) == 24 and cl[12:].all() and not cl[4:12].any() and ref['bw'][0].max() > 1.1
    assert float(np.median(ref['lp'][0][:, 19:])) == 0.0 and float(np.mean(ref['lp'][0][:, -4:] == 0.0)) > 0.95     # clipped at 0 dB SL but for the onset
    assert float(np.min(np.median(ref['lp'][0][:, 4:12], axis=0))) > 25.0
    # hearing loss: the table differs between x (normal hearing) and y, BWmin > 1, attnIHC > 0
    ref = C.reference('hl_mild_4801')
    assert not ref['loss'][0][0].any() and (ref['loss'][0][1] == 1.0).all() and (ref['loss'][1][1] > 1.0).all() and (ref['loss'][1][4] > 0).all()
    import make_golden_haspi
    assert tuple(make_golden_haspi.HL_MILD) == C.HL_MILD
    # dither: the active frames are not the first n_active frames, so "row k perturbs the k-th ACTIVE frame" differs from "frame k"
    ref = C.reference('dither_4803')
    assert ref['index'][0] > 0 and not np.array_equal(ref['index'], np.arange(ref['n_active']))
    plain = C.oracle_stages(*C.case('dither_4803')[:3])
    assert np.array_equal(plain['index'], ref['index']) and float(np.max(np.abs(plain['cep'] - ref['cep']))) > 0.05


def test_ragged_batch_layout():
    X, Y, lengths, rows = C.ragged()
    refs = C.ragged_reference()
    assert X.shape == Y.shape == (6, 5000) and tuple(lengths) == C.RAGGED_LENGTHS
    assert max(lengths) == X.shape[1] and min(lengths) == 2400
    assert sum(n % 9 == 1 for n in lengths) >= 1 and sum(n % 32 == 1 for n in lengths) >= 1
    for b, n in enumerate(lengths):
        assert np.isnan(X[b, n:]).all() and np.isnan(Y[b, n:]).all() and np.isfinite(X[b, :n]).all() and np.isfinite(Y[b, :n]).all()
        assert refs[b]['n_active'] > 1 and np.isfinite(refs[b]['raw'])
    assert [r['n_active'] for r in refs] == [545, 256, 434, 332, 504, 327]
    # rows that end inside the padded length's chunks: the chunk counts differ from row to row
    assert sorted({-(-int(n) // C.GS_LC) for n in lengths}) == [2, 3, 4]
