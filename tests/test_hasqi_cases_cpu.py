"""CPU: the premises of tests/test_haspi_quality_stages_gpu.py.  Every case of tests/hasqi_cases.py exists to put a seam of
csrc/haspi_quality.h under the comparison (a half-window segment, the last lag group, the tile's fallback rows, a block seam, a gate,
an empty loudness third); here every count is recomputed from the oracle and pinned, so that a case cannot silently stop exercising
its seam, and every gate decision is shown to be far from its threshold."""
import numpy as np
import pytest

import hasqi_cases as C

H = C.H
# name -> (n24, segments, above eb_melcor's gate, above the covariance gate, histogram bins, shift spread per group of 8 bands)
EXPECTED = {
    'min_2400': (2400, 12, 11, 11, 25, (260, 88, 51, 14)),
    'seg_2495': (2495, 12, 11, 11, 25, (260, 88, 51, 14)),
    'seg_2496': (2496, 13, 12, 12, 33, (260, 89, 51, 14)),
    'seg_2497': (2497, 13, 12, 12, 33, (260, 89, 51, 14)),
    'blocks_16385': (16385, 85, 84, 84, 47, (260, 89, 51, 14)),
    'long_49500': (49500, 257, 256, 256, 47, (261, 88, 51, 14)),
    'gap_12000': (12000, 62, 44, 44, 96, (260, 88, 51, 14)),
    'delay_p24': (5000, 26, 25, 25, 42, (260, 89, 51, 14)),
    'delay_p25': (5000, 26, 25, 25, 42, (260, 89, 51, 14)),
    'delay_m24': (5000, 26, 25, 25, 42, (260, 89, 51, 14)),
    'negated': (3000, 15, 14, 14, 32, (260, 88, 51, 14)),
    'same': (3000, 15, 14, 14, 32, (260, 88, 51, 14)),
    'steady_9600': (9600, 50, 49, 49, 31, (235, 118, 42, 15)),
    'wide_spread': (4000, 20, 19, 19, 43, (324, 69, 21, 6)),
    'in_tile': (4000, 20, 19, 19, 47, (235, 101, 43, 19)),
    'rs16k_9001': (13502, 70, 69, 69, 45, (260, 88, 51, 14)),
    'hl_mild_4801': (4801, 25, 24, 24, 58, (197, 78, 35, 11)),
    'hl_mild_4801_i0': (4801, 25, 24, 24, 42, (260, 89, 51, 14)),
    'hl_sloping_4801': (4801, 25, 24, 24, 51, (223, 94, 35, 7)),
}
PREMISE = 1e-6


def test_the_restated_constants_and_the_case_table():
    assert (C.HQ_NWIN, C.HQ_NHALF, C.HQ_MAXLAG, C.HQ_TROWS) == (384, 192, 24, 640)
    assert (C.GL_N, C.IHC_CHUNKS_PER_BLOCK, C.LOUD_SEGS_PER_BLOCK, C.FINAL_THREADS) == (2048, 8, 64, 256)
    assert C.BLOCKS_N == 16385 and sorted(C.CASES) == sorted(EXPECTED)
    assert round(16 * 0.001 * H.FSAMP) == C.HQ_NWIN and round(1.0 * 0.001 * H.FSAMP) == C.HQ_MAXLAG
    # 13 lag groups of 4 cover 52 slots for the 49 lags
    assert 13 * 4 >= 2 * C.HQ_MAXLAG + 1 > 12 * 4
    # the literal normalisers of hq_segment_kernel
    w = np.hanning(C.HQ_NWIN)
    assert np.isclose(w.sum(), 191.5, rtol=1e-14) and np.isclose(w[C.HQ_NHALF:].sum(), 95.75, rtol=1e-14)
    assert np.isclose((w ** 2).sum(), 143.625, rtol=1e-14) and np.isclose((w[C.HQ_NHALF:] ** 2).sum(), 71.8125, rtol=1e-14)


@pytest.mark.parametrize('name', sorted(EXPECTED))
def test_counts_and_gate_margins_of_a_case(name):
    n24, nseg, n_mel, n_cov, nbins, spread = EXPECTED[name]
    x, y, fs, HL, itype = C.case(name)
    r = C.reference(name)
    assert len(x) == len(y) == C.CASES[name][1] and x.dtype == y.dtype == np.float32
    assert C.n24_of(len(x), fs) == n24 == r['env'].shape[1]
    assert C.n_segments(n24) == nseg == H.n_segments(n24, C.HQ_NWIN) == r['sm'].shape[1] == r['cov'].shape[0]
    assert (r['n_mel'], r['n_cov'], r['nbins'], r['status']) == (n_mel, n_cov, nbins, 0)
    assert tuple(r['spread'].tolist()) == spread and int(r['shift'].min()) == 0
    # the gates: every segment loudness and every cell level away from 2.5 dB, every loudness away from the histogram's mid-points, every
    # cumulative share away from 0.333 and 0.667; no cell at the 1e-30 gate of the mean squares
    for k in ('margin_seg', 'margin_cell', 'margin_mid', 'margin_cum'):
        assert r[k] > PREMISE, (k, r[k])
    for k in ('msx', 'msy'):
        assert not np.any((r[k] > C.SMALL) & (r[k] < 4 * C.SMALL)), k
    assert np.isfinite(r['sm']).all() and np.isfinite(r['cov']).all() and np.all((r['cov'] >= 0) & (r['cov'] <= 1))


def test_the_segment_seams():
    last_end = {name: (EXPECTED[name][1] - 1) * C.HQ_NHALF + C.HQ_NHALF for name in ('min_2400', 'seg_2495', 'seg_2496', 'seg_2497')}
    assert last_end == {'min_2400': 2304, 'seg_2495': 2304, 'seg_2496': 2496, 'seg_2497': 2496}
    assert 2400 - last_end['min_2400'] == 96                      # a tail no segment reaches
    assert last_end['seg_2496'] == 2496                           # the last half window ends on the last sample
    # the half windows' samples matter: the first and the last smoothed values change when the window's other half is used
    r = C.reference('seg_2496')
    env = C.shifted(r['env'][0], r['shift'])
    w = np.hanning(C.HQ_NWIN)
    wrong_last = env[:, 2304:2496] @ w[C.HQ_NHALF:] / np.sum(w[C.HQ_NHALF:])
    assert np.max(np.abs(wrong_last - r['sm'][0][-1])) > 1e-2


def test_the_block_seams():
    n24, nseg = EXPECTED['blocks_16385'][:2]
    chunks = -(-n24 // C.GL_N)
    assert chunks == C.IHC_CHUNKS_PER_BLOCK + 1 and n24 - C.IHC_CHUNKS_PER_BLOCK * C.GL_N == 1      # a second IHC block that holds one sample
    assert -(-nseg // C.LOUD_SEGS_PER_BLOCK) == 2                                                     # a second loudness block
    assert EXPECTED['long_49500'][1] == C.FINAL_THREADS + 1                                           # one thread of the final kernel owns two segments
    assert all(EXPECTED[n][1] <= C.LOUD_SEGS_PER_BLOCK for n in ('min_2400', 'delay_p24', 'steady_9600'))


def test_the_gap_puts_segments_below_both_gates_and_cells_at_zero():
    r = C.reference('gap_12000')
    x, y = C.case('gap_12000')[:2]
    assert not x[:C.ZERO_HEAD].any() and not y[:C.ZERO_HEAD].any() and not x[C.ZERO_GAP[0]:C.ZERO_GAP[1]].any() and y[C.ZERO_GAP[0]:C.ZERO_GAP[1]].any()
    below = [0] + list(range(19, 36))
    assert np.where(r['segl'][0] <= C.GATE_DB)[0].tolist() == below and np.where(r['segl'][1] <= C.GATE_DB)[0].tolist() == below
    assert int(np.sum(r['msx'] == 0)) == 28 and int(np.sum((r['msx'] > 0) & (r['msx'] <= 2 * C.SMALL))) > 500
    dead = (r['msx'] <= 2 * C.SMALL) | (r['msy'] <= 2 * C.SMALL)
    assert np.all(r['cov'][dead] == 0) and np.all(r['cov'][~dead] > 0)


def test_the_delays_put_the_maximum_on_the_end_lags():
    """y = x delayed by d: the maximum sits at lag -d (x[n + l] against y[n]).  +24 and -24 are the first and the last lag of the search
    (the last one is the lone member of the thirteenth lag group); at 25 the peak is outside and the covariance falls."""
    stats = {}
    for name in ('delay_p24', 'delay_m24', 'delay_p25'):
        r = C.reference(name)
        lag = C.lag_argmax(C.shifted(r['bm'][0], r['shift']), C.shifted(r['bm'][1], r['shift']))
        live = r['msx'][1:-1] > C.GATE_DB ** 2
        stats[name] = (int(live.sum()), int(np.sum((lag == -24) & live)), int(np.sum((lag == 24) & live)), float(r['cov'][1:-1][live].mean()))
    assert stats['delay_p24'][:3] == (767, 760, 0) and stats['delay_m24'][:3] == (767, 3, 714) and stats['delay_p25'][:3] == (767, 250, 0)
    assert stats['delay_p24'][3] > 0.999 and stats['delay_m24'][3] > 0.99 and stats['delay_p25'][3] < 0.97
    assert C.reference('delay_p24')['Nonlin'] - C.reference('delay_p25')['Nonlin'] > 0.015          # a dropped end lag is visible in the score too


def test_negated_and_same_sit_on_the_clip():
    a, b = C.reference('same'), C.reference('negated')
    assert np.array_equal(a['cov'], b['cov']) and np.array_equal(a['msx'], a['msy']) and np.array_equal(b['msx'], b['msy'])
    assert int(np.sum(a['cov'] == 1.0)) == 433 and int(np.sum(a['cov'] > 0)) == 453
    assert a['CepCorr'] == pytest.approx(1.0, abs=1e-12) and b['Nonlin'] == pytest.approx(1.0, abs=1e-12)


def test_the_steady_tones_leave_the_lowest_loudness_third_empty():
    r = C.reference('steady_9600')
    x, y, fs, _HL, _it = C.case('steady_9600')
    assert np.isnan(r['cov3'][0]) and np.isfinite(r['cov3'][1:]).all() and np.isnan(r['Intel'])
    assert all(np.isfinite(r[k]) for k in ('CepCorr', 'avecov', 'sync5', 'Nonlin', 'Linear', 'Combined', 'Dloud', 'Dslope'))
    assert r['edges'][0] == 0.0                                    # no bin's cumulative share is below 0.333: the first bin holds more
    with np.errstate(invalid='ignore', divide='ignore'):
        v1, raw = H.haspi_v1(x, fs, y, fs)
    assert np.isnan(v1) and np.isnan(raw[1]) and raw[0] == r['CepCorr']


def test_the_tile_cases():
    """hq_segment_kernel's tile holds 640 rows = 384 + a spread of 256 inside a group of 8 bands; a wider group reads the rest from
    global memory."""
    room = C.HQ_TROWS - C.HQ_NWIN
    assert room == 256
    wide, tile = C.reference('wide_spread')['spread'], C.reference('in_tile')['spread']
    assert wide[0] >= 300 and wide[0] - room == 68 and np.all(wide[1:] <= room)
    assert np.all(tile <= room) and np.all(C.reference('steady_9600')['spread'] <= room)
    assert C.reference('min_2400')['spread'][0] - room == 4        # the usual signal: four rows per segment
    bw = C.reference('wide_spread')['bw'][0]
    BW1 = H.loss_parameters(100 * np.ones(6), H.center_freq())[1]
    assert bw[0] == 1.0 and bw[7] == BW1[7]


def test_the_sloping_loss_puts_high_band_cells_under_the_cell_gate():
    r = C.reference('hl_sloping_4801')
    rms = np.sqrt(r['msx'])
    assert int(np.sum((rms[:, 24:] < C.GATE_DB) & (rms[:, 24:] > 0))) == 192 and int(np.sum(rms[:, 24:] > C.GATE_DB)) == 0
    assert int(np.sum(np.abs(rms - C.GATE_DB) < 0.5)) == 12
    n = np.sqrt(C.reference('min_2400')['msx'])
    assert int(np.sum(np.abs(n - C.GATE_DB) < 0.5)) == 0


@pytest.mark.parametrize('name', ['min_2400', 'hl_sloping_4801', 'hl_mild_4801_i0', 'rs16k_9001'])
def test_the_restated_chain_is_the_oracles(name):
    """hasqi_cases.ear_bm (un-shifted outputs) shifted = oracle.ear_model_bm, bit for bit; the scores of oracle_stages are those of
    oracle.haspi_v1 / hasqi_v2."""
    x, y, fs, HL, itype = C.case(name)
    r = C.reference(name)
    xdB, xBM, ydB, yBM, xSL, ySL, p = H.ear_model_bm(r['r24'][0], H.FSAMP, r['r24'][1], H.FSAMP, HL=HL, itype=itype)
    sh = r['shift']
    assert np.array_equal(sh, p['shifts']) and np.array_equal(r['bw'], np.stack([p['BWx'], p['BWy']]))
    assert np.array_equal(C.shifted(r['env'][0], sh), xdB) and np.array_equal(C.shifted(r['env'][1], sh), ydB)
    assert np.array_equal(C.shifted(r['bm'][0], sh), xBM) and np.array_equal(C.shifted(r['bm'][1], sh), yBM)
    assert np.array_equal(r['sl'], np.stack([xSL, ySL]))
    if itype == 0:
        v1, raw = H.haspi_v1(x, fs, y, fs, HL=HL)
        assert v1 == r['Intel'] and raw[0] == r['CepCorr'] and np.array_equal(raw[1:], r['cov3'])
    if itype == 2 or HL is None:
        q = H.hasqi_v2(x, fs, y, fs, HL=HL)
        assert (q[0], q[1], q[2]) == (r['Combined'], r['Nonlin'], r['Linear']) and q[3] == [r['CepCorr'], r['sync5'], r['Dloud'], r['Dslope']]


def test_the_ragged_batch():
    X, Y, lengths, rows = C.ragged()
    assert tuple(lengths.tolist()) == C.RAGGED_LENGTHS == (5000, 2400, 2495, 2496, 2497, 4641) and X.shape == (6, 5000)
    assert lengths[5] % 32 == 1
    expected = [(26, 25, 25, 42), (12, 11, 11, 25), (12, 11, 11, 25), (13, 12, 12, 33), (13, 12, 12, 33), (24, 23, 23, 42)]
    for b, ((x, y), r) in enumerate(zip(rows, C.ragged_reference())):
        assert np.array_equal(X[b, :lengths[b]], x) and np.array_equal(Y[b, :lengths[b]], y)
        assert np.isnan(X[b, lengths[b]:]).all() and np.isnan(Y[b, lengths[b]:]).all()
        assert (r['sm'].shape[1], r['n_mel'], r['n_cov'], r['nbins']) == expected[b] and r['status'] == 0
        for k in ('margin_seg', 'margin_cell', 'margin_mid', 'margin_cum'):
            assert r[k] > PREMISE, (b, k, r[k])
