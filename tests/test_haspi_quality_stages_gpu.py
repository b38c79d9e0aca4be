"""GPU: every stage of csrc/haspi_quality.h (HASPI version 1 and HASQI v2 behind the shared ear model) against oracle/haspi.py (float64
numpy / scipy), row by row, read out of the workspace through nele_metric_haspi_quality_sections (metrics.haspi_quality_stages).  The
scores are means over hundreds of segments times 32 bands of correlations clipped to [0, 1]: a fault in one segment, one band or one lag
is averaged away there; the stages show it.  Cases and their premises: tests/hasqi_cases.py, tests/test_hasqi_cases_cpu.py.

Each stage is compared with the oracle's function of THAT stage, fed the kernel's own previous stage widened to float64 (the r24 device of
tests/test_haspi_stages_gpu.py): the stage gets a bound of its own, and every gate decision (segment loudness, cell level, histogram
bin, loudness third) is taken on the same numbers on both sides.  The ear model's outputs go against the oracle's chain started from the
float32 signals at 24 kHz that the kernel left.  u = 2^-24 is half a float32 ulp, relative.

Exact: shift, qinfo = {segments above eb_melcor's gate, status 0, above the covariance gate, len(bins)} (against the pure oracle and
against the oracle's back end run on the kernel's stages), info == qinfo, the NaN pattern of the twelve outputs, cells with a mean square
<= 1e-30 are 0 in msx / msy / cov on both sides, 0 <= cov <= 1.  A NaN (the 0xFF fill) anywhere inside a row's extent fails.

Bounds in force and where they come from ("measured" = the worst over all cases and ragged rows on an MI355X, with its case):
  env    1.24e-4 dB = 2 x haspi_cases.ENV_DB + 2^-18: the budget of the dB-SL envelope through the IHC adaptation's output gain R1inv = 2,
         and the float32 rounding of the adapted value (< 128 dB); no window.  measured 4.4e-5 dB (blocks_16385, y).  4 x the measured
         worst would be above the budget: the budget is asserted
  bm     per sample, budget(env) + 2^-23 (|adapted envelope| + budget(env)): BM = (adapted + 1e-30) cos(phase); the envelope's error times
         |cos| <= 1, the float32 roundings of cos(phase) and of the product (u each, of values <= the envelope).
         measured 0.35 of the bound, 4.5e-5 absolute (in_tile)
  sm     384 x 2^-52 x max|env| of the row (5e-12): a float64 sum of 384 products with a window of unit sum.  measured 4.3e-14 (steady_9600)
  msx, msy   (2^-23 + 800 x 2^-53) relative + 1e-38: each windowed, mean-removed sample is rounded ONCE to float32 (u), its square moves
         by 2 u; float64 sums of <= 384 terms twice (mean, squares); 1e-38 for samples below 2^-126, eight decades under the 1e-30
         gate.  This is the bound of the float32 storage of the segments.  measured 0.70 of the bound = 8.4e-8 relative (wide_spread)
  cov    (2^-23 + 800 x 2^-53) (R + 1) = 2.7e-7 with R = max_l xcorr(w, w, 0) / xcorr(w, w, l) over |l| <= 24 (lag_ratio(): the half window
         decides): the lag sum moves by 2 u sum|x||y| <= 2 u sqrt(Sxx Syy) (Cauchy-Schwarz), which the normalisation turns into 2 u R;
         sqrt(MSx MSy) moves by 2 u relative, and cov <= 1.  The clip does not enlarge a difference.  measured 1.9e-8 (wide_spread)
  corr   384 x 2^-53 = 4.3e-14 relative: a float64 sum of <= 384 positive products.  measured 1.6e-15 (seven ulps)
  segl   1e-13 dB: 20 / ln 10 x (32 terms + 2 x 12 for the exponent's rounding at |arg| < 12 + 4) x 2^-53 = 5.8e-14.  measured 1.4e-14
         (blocks_16385)
  CepCorr, cov3, avecov, BMsync5   1e-10: float64 sums of <= 257 x 32 terms (9e-13 relative); the variance sums of eb_melcor cancel by
         (level / spread)^2 <= 100.  measured 7.8e-16 (CepCorr, seg_2496), 3.3e-16 for the covariance averages
  sl     1.2e-6 dB = 4 x measured 3.0e-7 dB (in_tile; 2.4e-7 in nearly every case, x and y alike), never above sl_budget() = 2.5e-6 dB.  The
         sums of |u|^2 are float64 on both sides; what shows is the reference's own 4th-order section with a fourfold pole a, whose
         response 1 / (1 - a)^4 moves by up to 15 x 2^-53 / (1 - a)^4 = 2.7e-7 relative in the lowest band with the last bit of exp()
         (device against libm), as for 'bw' in tests/test_haspi_stages_gpu.py
  Dloud, Dslope, Linear, Nonlin, Combined, Intel   1e-12 absolute from the kernel's own sl / CepCorr / BMsync5 / cov3: a few dozen
         float64 operations on values <= 1 (Dloud: 32 x std / 2.5 of differences of normalised spectra).  measured 1.6e-15 (Dslope, in_tile)
The gates on the kernel's own values: every margin above 1e-9 is asserted; measured 0.067 dB (segment loudness, gap_12000), 1.6e-4 dB (cell
level, steady_9600), 1.8e-4 dB (histogram mid-point, delay_m24), 3.3e-4 (cumulative share: 1/3 against 0.333).
The noise (test_the_bm_noise_...): bounds from the sample count and the float32 quantisation of the noisy sample (moments()); measured on
153 600 samples: mean 5e-4 / 0.021, variance - 1 1.6e-3 / 0.037, fourth moment - 3 0.030 / 0.23, max |z| 4.71 / 5.77, correlations <= 3.4e-3
against 9e-3 .. 1.8e-2.
The end-to-end comparisons of tests/test_haspi_quality_gpu.py and tests/test_hasqi_target_gpu.py (rtol 2e-5 .. 1e-4 on the final numbers)
stay as they are; nothing measured here contradicts the tolerances they or csrc/haspi_quality.h state (the float32 storage shows as
1e-7 relative in msx and 2e-8 in cov; phase 0 and the one-shot call differ by one ulp in the scores, inside their rtol 1e-9).

One-line faults tried against these tests (never committed): the last lag dropped, the tile's fallback read zeroed, the last segment's
window offset, the loudness-third edge comparison, the half-window normaliser; what caught each - and why no input of at most 49 500 samples
can catch the fourth - is recorded in docs/LAB_NOTEBOOK.md."""
import numpy as np
import pytest

import hasqi_cases as C

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
H = C.H

U32 = 2.0 ** -24
ENV_DB = 2 * C.HC.ENV_DB + 2.0 ** -18
MS_REL = 2.0 ** -23 + 800 * 2.0 ** -53
MS_TINY = 1e-38                    # float32 underflow of a windowed sample below 2^-126: eight decades under the 1e-30 gate
CORR_REL = 384 * 2.0 ** -53
SEGL_DB = 1e-13
BACK_ABS = 1e-10
SL_DB = 1.2e-6
SCORE_ABS = 1e-12
MARGIN = 1e-9                      # the gates, on the kernel's own values: far above the float64 bounds, far below the 1e-6 premise
V1_COLS = ('Intel', 'CepCorr', 'cov3_0', 'cov3_1', 'cov3_2', 'Combined', 'Nonlin', 'Linear', 'sync5', 'Dloud', 'Dslope', 'avecov')
V2_COLS = ('Combined', 'Nonlin', 'Linear', 'CepCorr', 'sync5', 'Dloud', 'Dslope')
STAGES = ('r24', 'rinfo', 'bw', 'shift', 'env', 'bm', 'sse', 'ssp', 'sm', 'cov', 'msx', 'msy', 'segl', 'qinfo', 'sl')


def lag_ratio():
    """R of the docstring for the full and the half window"""
    w = np.hanning(C.HQ_NWIN)
    return max(float(np.max(H.window_corr(v, C.HQ_MAXLAG)) * np.sum(v ** 2)) for v in (w, w[C.HQ_NHALF:]))


COV_ABS = MS_REL * (lag_ratio() + 1)


def sl_budget():
    """The a-priori bound on a band level of eb_aveSL, in dB: the sensitivity of the reference's 4th-order sections with a FOURFOLD pole a to
    the last bit of their coefficients (tests/test_haspi_stages_gpu.py, bw_budget): the level of the signal bank at BW >= 1, plus the
    control bank's at BW1 times the compression slope 1 - 1 / CR; the lowest band (a = 0.9912) decides."""
    cf = H.center_freq()
    _aO, _bw, _lk, CR, _aI = H.loss_parameters(np.zeros(6), cf)
    BW1 = H.loss_parameters(100 * np.ones(6), cf)[1]

    def sens(BW):
        a = np.exp(-BW * 2 * np.pi / H.FSAMP * (24.7 + cf / 9.26449) * 1.019)
        return (4 * a + 6 * a ** 2 + 4 * a ** 3 + a ** 4) * 2.0 ** -53 / (1 - a) ** 4
    return float(np.max(20 / np.log(10.0) * (sens(np.ones(len(cf))) + (1 - 1 / CR) * sens(BW1))))


SL_DB_PRIORI = sl_budget()


@pytest.fixture(scope='module')
def mt():
    assert torch.cuda.is_available()
    from nele_gan_amd import metrics
    return metrics


def maxabs(a):
    a = np.asarray(a)
    return float(np.max(np.abs(a))) if a.size else 0.0


def flat(o):
    """back_end()'s dict -> {column name: value}"""
    d = {k: float(o[k]) for k in ('Intel', 'CepCorr', 'Combined', 'Nonlin', 'Linear', 'sync5', 'Dloud', 'Dslope', 'avecov')}
    d.update({'cov3_%d' % j: float(o['cov3'][j]) for j in range(3)})
    return d


def compare(tag, out, info, st, b, pure, HL, itype, cols=V1_COLS, check=True):
    """Row b of haspi_quality_stages' output against the oracle stage by stage; prints each figure with its bound, then asserts."""
    got = {k: st[k][b] for k in STAGES}
    problems = []

    def want(ok, what):
        if not ok:
            problems.append(what)
    for k in ('r24', 'env', 'bm', 'sm', 'cov', 'msx', 'msy', 'segl', 'sl', 'sse', 'ssp', 'bw'):
        want(bool(np.isfinite(got[k]).all()), (k, 'not finite: %d values' % int(np.count_nonzero(~np.isfinite(got[k])))))
    want(bool(np.isfinite(st['corr']).all()), 'corr not finite')
    if problems:
        assert not check, (tag, problems)
        print('   PROBLEMS', tag, problems)
        return {}
    ref = C.oracle_stages(None, None, 24000, HL, itype, r24=got['r24'])      # the oracle's chain from the kernel's signals at 24 kHz
    sh = got['shift']
    want(np.array_equal(sh, ref['shift']) and np.array_equal(sh, pure['shift']), ('shift', sh.tolist(), pure['shift'].tolist()))
    fig = {}
    env, bm = got['env'].astype(np.float64), got['bm'].astype(np.float64)
    for s in range(2):
        fig['env[%d]' % s] = (maxabs(env[s] - ref['env'][s]), ENV_DB)
        bound = ENV_DB + 2 * U32 * (np.abs(ref['env'][s]) + ENV_DB)
        fig['bm[%d]' % s] = (float(np.max(np.abs(bm[s] - ref['bm'][s]) / bound)), 1.0)
    fig['bm abs'] = (maxabs(bm - ref['bm']), np.inf)
    # eb_EnvSmooth and eb_BMcovary of the kernel's own shifted arrays
    for s in range(2):
        fig['sm[%d]' % s] = (maxabs(got['sm'][s] - H.env_smooth(C.shifted(env[s], sh)).T), 384 * 2.0 ** -52 * maxabs(env[s]))
    cov, msx, msy = (a.T for a in H.bm_covary(C.shifted(bm[0], sh), C.shifted(bm[1], sh)))
    for k, r in (('msx', msx), ('msy', msy)):
        want(np.array_equal(got[k] == 0, r == 0), (k, 'zero cells differ'))
        want(not np.any((r > C.SMALL) & (r < 4 * C.SMALL)), (k, 'a cell at the 1e-30 gate'))
        fig[k] = (float(np.max(np.abs(got[k] - r) / (MS_REL * r + MS_TINY))), 1.0)
    dead = (msx <= 2 * C.SMALL) | (msy <= 2 * C.SMALL)
    want(bool(np.all(got['cov'][dead] == 0)) and bool(np.all(cov[dead] == 0)), 'cov of a cell without a mean square')
    want(bool(np.all((got['cov'] >= 0) & (got['cov'] <= 1))), 'cov outside [0, 1]')
    fig['cov'] = (maxabs(got['cov'] - cov), COV_ABS)
    w = np.hanning(C.HQ_NWIN)
    for j, v in enumerate((w, w[C.HQ_NHALF:])):
        r = H.window_corr(v, C.HQ_MAXLAG)
        fig['corr[%d]' % j] = (float(np.max(np.abs(st['corr'][j] - r) / r)), CORR_REL)
    # the back end from the kernel's own sm, cov, msx and sl
    be = C.back_end(got['sm'], got['cov'], got['msx'], got['sl'])
    fig['segl'] = (maxabs(got['segl'] - be['segl']), SEGL_DB)
    for k in ('margin_seg', 'margin_cell', 'margin_mid', 'margin_cum'):
        want(be[k] > MARGIN, (k, be[k]))
    qi = [be['n_mel'], be['status'], be['n_cov'], be['nbins']]
    pq = [pure['n_mel'], pure['status'], pure['n_cov'], pure['nbins']]
    want(got['qinfo'].tolist() == qi == pq and info[b].tolist() == qi, ('qinfo', got['qinfo'].tolist(), info[b].tolist(), qi, pq))
    exp = flat(be)
    o = dict(zip(cols, out[b]))
    want(all(np.isnan(o[k]) == np.isnan(exp[k]) for k in cols), ('NaN pattern', o, exp))
    for k in cols:
        if k in ('CepCorr', 'sync5', 'avecov') or k.startswith('cov3'):
            fig[k] = (0.0 if np.isnan(exp[k]) else abs(o[k] - exp[k]), BACK_ABS)
    for s in range(2):
        fig['sl[%d]' % s] = (maxabs(got['sl'][s] - ref['sl'][s]), min(SL_DB, SL_DB_PRIORI))
    # the score formulas from the kernel's own components
    fig['Dloud'] = (abs(o['Dloud'] - exp['Dloud']), SCORE_ABS)
    fig['Dslope'] = (abs(o['Dslope'] - exp['Dslope']), SCORE_ABS)
    lin = 0.579 * o['Dloud'] + 0.421 * o['Dslope']
    non = (o['CepCorr'] ** 2) * o['sync5']
    fig['Linear'] = (abs(o['Linear'] - lin), SCORE_ABS)
    fig['Nonlin'] = (0.0 if np.isnan(non) else abs(o['Nonlin'] - non), SCORE_ABS)
    fig['Combined'] = (0.0 if np.isnan(non) else abs(o['Combined'] - non * lin), SCORE_ABS)
    if 'Intel' in o:
        intel = 1.0 / (1.0 + np.exp(-(-9.047 + 14.816 * o['CepCorr'] + ((0.0 * o['cov3_0'] + 0.0 * o['cov3_1']) + 4.616 * o['cov3_2']))))
        fig['Intel'] = (0.0 if np.isnan(intel) else abs(o['Intel'] - intel), SCORE_ABS)
    print('%s: qinfo %s spread %s margins %.2g %.2g %.2g %.2g ' % (tag, qi, C.group_spread(sh).tolist(), be['margin_seg'], be['margin_cell'],
                                                              be['margin_mid'], be['margin_cum']) +
          ' '.join('%s %.3g/%.3g' % (k, e, bd) for k, (e, bd) in fig.items()))
    if check:
        assert not problems, (tag, problems)
        for k, (e, bd) in fig.items():
            assert e <= bd, (tag, k, e, bd)
    elif problems:
        print('   PROBLEMS', tag, problems)
    return fig


@pytest.mark.parametrize('name', sorted(C.CASES))
def test_every_stage_of_a_single_utterance(mt, name):
    """One utterance per call (B = 1, no lengths) through nele_metric_haspi_quality[_hl]: the segment seams, the block seams of every
    kernel, exact zeros, the end lags, the clip, an empty loudness third, the tile's fallback, the resampler, audiograms
    (see hasqi_cases.py)."""
    x, y, fs, HL, itype = C.case(name)
    out, info, st = mt.haspi_quality_stages(np.array(x)[None], np.array(y)[None], fs, HL=HL, itype=itype)
    compare(name, out, info, st, 0, C.reference(name), HL, itype)


@pytest.fixture(scope='module')
def ragged_runs(mt):
    X, Y, lengths, _rows = C.ragged()
    return {split: mt.haspi_quality_stages(np.array(X), np.array(Y), 24000, lengths=np.array(lengths), split=split) for split in (None, 'phase0', '3+4')}


def test_every_stage_of_every_row_of_a_ragged_batch(ragged_runs):
    """Six rows in one padded call (5000 = the padded length, 2400 = the minimum, 2495 / 2496 / 2497 around the thirteenth segment, 4641 =
    1 mod 32), NaN behind every row's end in x and y.  Every stage of every row equals the oracle on the cut row, in the one-shot call
    and in nele_metric_hasqi_var: a read past a row's end would show as NaN."""
    _X, _Y, lengths, _rows = C.ragged()
    pures = C.ragged_reference()
    for split, cols in ((None, V1_COLS), ('phase0', V2_COLS)):
        out, info, st = ragged_runs[split]
        for b in range(len(lengths)):
            compare('ragged[%d] len %d %s' % (b, lengths[b], split), out, info, st, b, pures[b], None, 0, cols=cols)


def test_rows_of_a_ragged_batch_score_as_they_do_alone(mt, ragged_runs):
    """Bit-identical scores: each row scored in a call of its own at its own length."""
    out, _info, _st = ragged_runs[None]
    out2, _info2, _st2 = ragged_runs['phase0']
    _X, _Y, lengths, rows = C.ragged()
    for b, (x, y) in enumerate(rows):
        alone = mt.batch_haspi_quality(np.array(x), np.array(y), 24000, noise=False).cpu().numpy()[0]
        alone2 = mt.batch_hasqi(np.array(x), np.array(y), 24000, noise=False).cpu().numpy()[0]
        print(b, int(lengths[b]), out[b].tolist(), alone.tolist())
        assert np.array_equal(alone.view(np.uint64), out[b].view(np.uint64)), (b, out[b], alone)
        assert np.array_equal(alone2.view(np.uint64), out2[b].view(np.uint64)), (b, out2[b], alone2)


def test_the_split_call_leaves_the_stages_of_phase_0_bit_for_bit(ragged_runs):
    """MODE 1 + MODE 2 of hq_segment_kernel (phase 3 then phase 4) against MODE 0 (phase 0): every stage of every row, the scores and info,
    bit for bit.  Phase 0 against the one-shot call: the stages up to the segment loudness come from the same kernels (bit for bit); the
    two instantiations of hq_final_kernel agree to a few ulps (rtol 1e-9, as tests/test_hasqi_target_gpu.py compares them)."""
    a = ragged_runs['phase0']
    for other in ('3+4', None):
        o = ragged_runs[other]
        if other is None:
            np.testing.assert_allclose(a[0], o[0][:, [5, 6, 7, 1, 8, 9, 10]], rtol=1e-9)
            for b in range(len(a[2]['sl'])):
                np.testing.assert_allclose(a[2]['sl'][b], o[2]['sl'][b], rtol=1e-12)
        else:
            assert np.array_equal(a[0].view(np.uint64), o[0].view(np.uint64)), other
        assert np.array_equal(a[1], o[1]), other
        for k in STAGES:
            if other is None and k == 'sl':
                continue
            for b in range(len(a[2][k])):
                ga, go = np.ascontiguousarray(a[2][k][b]), np.ascontiguousarray(o[2][k][b])
                assert ga.shape == go.shape and ga.dtype == go.dtype and ga.tobytes() == go.tobytes(), (other, k, b)
        assert a[2]['corr'].tobytes() == o[2]['corr'].tobytes() and a[2]['loss'].tobytes() == o[2]['loss'].tobytes(), other


def test_a_second_phase_4_leaves_the_clean_sections_as_they_were(mt):
    """Every byte nele_metric_hasqi_clean_sections names is the same after phase 3, after phase 4 and after a second phase 4 with
    another y."""
    import ctypes
    from nele_gan_amd import _lib
    X, Y, lengths, _rows = C.ragged()
    B, L = X.shape
    Xd, Yd = torch.from_numpy(np.nan_to_num(np.array(X))).cuda(), torch.from_numpy(np.nan_to_num(np.array(Y))).cuda()
    sp = mt.HasqiSplit(Xd, fs=24000, lengths=torch.from_numpy(np.array(lengths)), ws_kind='hasqi_stage_test')
    sp.ws.fill_(255)
    buf = (ctypes.c_longlong * 72)()
    n = _lib.lib.nele_metric_hasqi_clean_sections(B, L, 24000, buf, 24)
    assert n == 12
    sec = [(int(buf[3 * k]), int(buf[3 * k + 1]), int(buf[3 * k + 2])) for k in range(n)]

    def snap():
        return [sp.ws[o:o + nb].cpu().numpy().copy() if stv == 0 else sp.ws[o:o + B * stv].view(B, stv)[:, :nb].cpu().numpy().copy() for (o, stv, nb) in sec]
    sp.clean_part()
    s3 = snap()
    o1 = sp.degraded_part(Yd).cpu().numpy()
    s4 = snap()
    o2 = sp.degraded_part((0.5 * Xd + 0.5 * Yd).contiguous()).cpu().numpy()
    s5 = snap()
    o3 = sp.degraded_part(Yd).cpu().numpy()
    for k in range(n):
        assert np.array_equal(s3[k], s4[k]) and np.array_equal(s3[k], s5[k]), ('section', k, sec[k])
    assert np.isfinite(o1).all() and not np.array_equal(o1, o2) and np.array_equal(o1.view(np.uint64), o3.view(np.uint64))


def noise_pair():
    """Rows 1 and 2 of the ragged batch (2400 and 2495 samples) in one padded call, NaN behind each row's end"""
    X, Y, lengths, _rows = C.ragged()
    return np.array(X[1:3, :2495]), np.array(Y[1:3, :2495]), np.array(lengths[1:3])


def moments(tag, z, e):
    """Standard-normal checks of the noise z (all in-row samples) whose observed values carry a quantisation of at most e per sample
    (half a float32 ulp of the noisy BM sample, in units of the noise's scale): mean, variance and fourth moment within five standard
    errors of their estimators (1 / sqrt n, sqrt(2 / n), sqrt(96 / n)) plus what the quantisation can add (mean |e| on the mean;
    Minkowski on the second and fourth moments), and |z| <= sqrt(2 ln 2^24) + e (Box-Muller from a 24-bit uniform in (0, 1])."""
    n = z.size
    e1, e2, e4 = float(np.mean(e)), float(np.sqrt(np.mean(e ** 2))), float(np.mean(e ** 4) ** 0.25)
    m, m2, m4 = float(np.mean(z)), float(np.mean(z ** 2)), float(np.mean(z ** 4))
    b1 = 5 / np.sqrt(n) + e1
    s2 = 1 + 5 * np.sqrt(2.0 / n)
    b2 = 5 * np.sqrt(2.0 / n) + 2 * np.sqrt(s2) * e2 + e2 ** 2 + b1 ** 2
    s4 = 3 + 5 * np.sqrt(96.0 / n)
    b4 = (s4 ** 0.25 + e4) ** 4 - 3
    top = float(np.max(np.abs(z) - e))
    print('%s: n %d mean %.3g/%.3g var-1 %.3g/%.3g m4-3 %.3g/%.3g max|z| %.4f/%.4f quantisation mean %.3g max %.3g' % (
        tag, n, m, b1, m2 - m * m - 1, b2, m4 - 3, b4, top, np.sqrt(2 * np.log(2.0 ** 24)), e1, float(np.max(e))))
    assert abs(m) <= b1 and abs(m2 - m * m - 1) <= b2 and abs(m4 - 3) <= b4, tag
    assert top <= np.sqrt(2 * np.log(2.0 ** 24)) * (1 + 1e-6), tag


def noise_of(mt, X, Y, lengths, noise, seed, ids=None):
    """-> per row: (z [2, n24, 32] = (BM with noise - BM without) / 10^(-75/20), e = its quantisation bound, the noisy BM itself)"""
    gn = 10.0 ** (-75.0 / 20.0)
    kw = dict(lengths=lengths, split=None if noise is True else 'phase0')
    quiet = mt.haspi_quality_stages(X, Y, 24000, **kw)[2]['bm']
    loud = mt.haspi_quality_stages(X, Y, 24000, noise=noise, seed=seed, utt_ids=ids, **kw)[2]['bm']
    rows = []
    for q, v in zip(quiet, loud):
        assert np.isfinite(q).all() and np.isfinite(v).all()
        z = (v.astype(np.float64) - q.astype(np.float64)) / gn
        rows.append((z, U32 * (np.abs(v.astype(np.float64)) + 2.0 ** -126) * (1 + 2 * U32) / gn + 2 * U32 * np.abs(z), v))
    return rows


def decorrelated(tag, a, b):
    n = a.size
    r = float(np.mean(a * b) - np.mean(a) * np.mean(b)) / float(np.std(a) * np.std(b))
    print('%s: n %d corr %.3g/%.3g' % (tag, n, r, 5 / np.sqrt(n)))
    assert abs(r) <= 5 / np.sqrt(n), tag


@pytest.mark.parametrize('noise', [True, 'utterance'])
def test_the_bm_noise_is_standard_normal_white_and_keyed_as_documented(mt, noise):
    """eb_BMaddnoise from the counter-based generator: noise 1 (keyed by the row) through nele_metric_haspi_quality, noise 2 (keyed by
    the utterance id) through nele_metric_hasqi_var, on min_2400 alone and on a ragged pair."""
    x, y = C.case('min_2400')[:2]
    X, Y, lengths = noise_pair()
    ids = np.array([41, 42])
    runs = [('min_2400', noise_of(mt, np.array(x)[None], np.array(y)[None], None, noise, 5, ids[:1])),
            ('pair', noise_of(mt, X, Y, lengths, noise, 5, ids))]
    for tag, rows in runs:
        z = np.concatenate([r[0].ravel() for r in rows])
        e = np.concatenate([r[1].ravel() for r in rows])
        moments('%s noise %s' % (tag, noise), z, e)
        decorrelated('%s x against y' % tag, np.concatenate([r[0][0].ravel() for r in rows]), np.concatenate([r[0][1].ravel() for r in rows]))
        decorrelated('%s neighbouring bands' % tag, np.concatenate([r[0][:, :, :-1].ravel() for r in rows]),
                     np.concatenate([r[0][:, :, 1:].ravel() for r in rows]))
        decorrelated('%s neighbouring samples' % tag, np.concatenate([r[0][:, :-1].ravel() for r in rows]),
                     np.concatenate([r[0][:, 1:].ravel() for r in rows]))
    # the same two utterances with their rows swapped
    swapped = noise_of(mt, X[::-1].copy(), Y[::-1].copy(), lengths[::-1].copy(), noise, 5, ids[::-1].copy())
    pair = runs[1][1]
    for b in range(2):
        same = pair[b][2].tobytes() == swapped[1 - b][2].tobytes()
        assert same == (noise == 'utterance'), (noise, b, same)
    other = noise_of(mt, X, Y, lengths, noise, 6, ids)
    assert all(pair[b][2].tobytes() != other[b][2].tobytes() for b in range(2))           # the seed is part of the key
