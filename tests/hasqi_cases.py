"""Inputs and float64 references of the HASPI v1 / HASQI v2 stage tests (tests/test_haspi_quality_stages_gpu.py on the device,
tests/test_hasqi_cases_cpu.py for the premises).  Plain module: numpy and oracle/haspi.py only (and haspi_cases.am_pair), nothing here
touches a GPU and nothing is read from a file.

The lengths and signals come from the seams of csrc/haspi_quality.h (the constants below restate its #defines and launch shapes;
test_hasqi_cases_cpu.py recomputes every count).  All inputs are at 24 kHz unless named otherwise:
  min_2400            the shortest accepted signal: 12 segments, and a tail of 96 samples that the last half window does not reach
  seg_2495/6/7        12 / 13 / 13 segments; at 2496 the last half window ends on the last sample
  blocks_16385        8 IHC chunks of 2048 + 1 sample: a second block of hq_ihc_bm_kernel that holds ONE sample; 85 segments: a second
                      block of hq_loud_kernel
  long_49500          257 segments: thread 0 of hq_final_kernel owns two of them
  gap_12000           exact zeros in the first 50 samples of x AND y and over [3000, 7000) of x: segments below both silence gates, cells
                      with a mean square of exactly 0
  delay_p24/p25/m24   y = x delayed by +24, +25, -24 samples: the end lags of eb_BMcovary's search on each side, and the first outside
  negated, same       y = -x, y = x: the covariance depends on |c|; the ratio is clipped at 1, where rounding can exceed it
  steady_9600         two steady tones: the lowest loudness third of eb_3LevelCovary is empty (cov3[0] = 0 / 0 = NaN, HASPI v1 NaN)
  wide_spread         tones from 300 Hz up, heard (itype 2) with no loss at 250 Hz and 60 dB from 500 Hz on: band 0 stays at BWmin = 1 and
                      band 7 sits at BWmin = BW1 = 1.7, a shift spread of 324 in band group 0 (68 rows per segment take the global-memory
                      fallback of hq_segment_kernel's tile).  With normal hearing no signal gets there: a band reaches BW1 at 100 dB only,
                      and the input is normalised to 65 dB
  in_tile             low tones only: every group of 8 bands has a spread of at most 256 (no fallback row at all)
  rs16k_9001          16 kHz, odd L, n24 = 13502
  hl_mild_4801 (itype 2), hl_mild_4801_i0 (itype 0), hl_sloping_4801 (itype 2)   the audiograms of tests/golden/make_golden_haspi.py
and ragged(): six rows of different lengths in one padded call, NaN behind every row's end."""
import functools

import numpy as np

import haspi_cases as HC
from oracle import haspi as H

# csrc/haspi_quality.h, csrc/haspi.hip
HQ_NWIN, HQ_NHALF, HQ_MAXLAG, HQ_TROWS = 384, 192, 24, 640
GL_N, IHC_CHUNKS_PER_BLOCK, LOUD_SEGS_PER_BLOCK, FINAL_THREADS = 2048, 8, 64, 256
HL_MILD = HC.HL_MILD
HL_SLOPING = (10.0, 15.0, 30.0, 50.0, 70.0, 80.0)      # tests/golden/make_golden_haspi.py
HL_WIDE = (0.0, 60.0, 60.0, 60.0, 60.0, 60.0)
GATE_DB = 2.5
SMALL = 1.0e-30
BLOCKS_N = GL_N * IHC_CHUNKS_PER_BLOCK + 1

# name -> (fs, L, audiogram or None, itype)
CASES = {
    'min_2400': (24000, 2400, None, 0), 'seg_2495': (24000, 2495, None, 0), 'seg_2496': (24000, 2496, None, 0),
    'seg_2497': (24000, 2497, None, 0), 'blocks_%d' % BLOCKS_N: (24000, BLOCKS_N, None, 0), 'long_49500': (24000, 49500, None, 0),
    'gap_12000': (24000, 12000, None, 0), 'delay_p24': (24000, 5000, None, 0), 'delay_p25': (24000, 5000, None, 0),
    'delay_m24': (24000, 5000, None, 0), 'negated': (24000, 3000, None, 0), 'same': (24000, 3000, None, 0),
    'steady_9600': (24000, 9600, None, 0), 'wide_spread': (24000, 4000, HL_WIDE, 2), 'in_tile': (24000, 4000, None, 0),
    'rs16k_9001': (16000, 9001, None, 0), 'hl_mild_4801': (24000, 4801, HL_MILD, 2), 'hl_mild_4801_i0': (24000, 4801, HL_MILD, 0),
    'hl_sloping_4801': (24000, 4801, HL_SLOPING, 2),
}
ZERO_HEAD, ZERO_GAP = 50, (3000, 7000)
DELAYS = {'delay_p24': 24, 'delay_p25': 25, 'delay_m24': -24}
RAGGED_LENGTHS = (5000, 2400, 2495, 2496, 2497, 4641)           # 4641 % 32 == 1, 5000 = the padded length
WIDE_TONES = (300.0, 520.0, 930.0, 1870.0, 3100.0, 5200.0)
TILE_TONES = (90.0, 150.0, 230.0)


def n_segments(n24):
    return 1 + n24 // HQ_NWIN + (n24 - HQ_NHALF) // HQ_NWIN


def n24_of(L, fs):
    return HC.dims(L, fs)[0]


def delayed(x, d):
    """x delayed by d samples (d < 0: advanced), zeros shifted in, the length kept"""
    if d >= 0:
        return np.concatenate((np.zeros(d, dtype=x.dtype), x[:len(x) - d]))
    return np.concatenate((x[-d:], np.zeros(-d, dtype=x.dtype)))


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (x, y, fs, HL or None, itype)"""
    fs, L, HL, itype = CASES[name]
    if name == 'steady_9600':
        t = np.arange(L) / float(fs)
        x = 0.3 * np.sin(2 * np.pi * 1000.0 * t) + 0.2 * np.sin(2 * np.pi * 2500.0 * t + 1.0)
        y = x + 0.02 * np.random.default_rng(9600).standard_normal(L)
        x, y = x.astype(np.float32), y.astype(np.float32)
    elif name == 'wide_spread':
        x, y = HC.am_pair(L, fs, 311, tones=WIDE_TONES, noise=0.0005, snr_noise=0.1)
    elif name == 'in_tile':
        x, y = HC.am_pair(L, fs, 312, tones=TILE_TONES, noise=0.0, snr_noise=0.002)
    else:
        x, y = HC.am_pair(L, fs, 7000 + L)
    if name == 'gap_12000':
        x[:ZERO_HEAD] = 0.0
        y[:ZERO_HEAD] = 0.0
        x[ZERO_GAP[0]:ZERO_GAP[1]] = 0.0
    if name in DELAYS:
        y = delayed(x, DELAYS[name])
    if name == 'negated':
        y = -x
    if name == 'same':
        y = x.copy()
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y, fs, HL, itype


def normalised_r24(x, y, fs):
    """The float32 signals at 24 kHz that the ear model starts from (pyhaspi2.py:81-84, :810-821): [2, n24] float32"""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    L = min(len(x), len(y))
    x, y = x[:L], y[:L]
    x = x / np.sqrt(np.sum(x ** 2) / L)
    y = y / np.sqrt(np.sum(y ** 2) / L)
    return np.stack([H.resample_24k(x, fs), H.resample_24k(y, fs)]).astype(np.float32)


def ear_bm(r24, HL=None, itype=0):
    """oracle.ear_model_bm (pyhaspi2.py:1155-1248) restated from its own per-channel functions, run from signals at 24 kHz, with the
    envelope and the BM motion BEFORE the group-delay shift (the kernels store them so and shift on load; ear_model_bm's shift drops the
    last shift[c] samples of channel c): -> dict(env [2, n24, 32] adapted envelope in dB SL, bm [2, n24, 32], sl [2, 32], shift [32],
    bw [2, 32]).  test_hasqi_cases_cpu.py checks that shifted(env), shifted(bm), sl, bw and shift equal ear_model_bm's bit for bit."""
    r24 = np.asarray(r24, dtype=np.float32)
    small = SMALL
    cfreq = H.center_freq()
    lossp = H._loss_pair(HL, itype)
    BW1 = H.loss_parameters(100 * np.ones(6), cfreq)[1]
    n = r24.shape[1]
    mid = (H.middle_ear(r24[0]), H.middle_ear(r24[1]))
    env = np.zeros((2, n, H.NCHAN))
    bm = np.zeros((2, n, H.NCHAN))
    ave, cave, BW = np.zeros((2, H.NCHAN)), np.zeros((2, H.NCHAN)), np.zeros((2, H.NCHAN))
    for c in range(H.NCHAN):
        coscf, sincf = H.cos_sin_cf(n, H.FSAMP, cfreq[c])
        for s in range(2):
            attnOHC, BWmin, lowknee, CR, attnIHC = lossp[s]
            control = H.gammatone_env(mid[s], BW1[c], coscf, sincf, cfreq[c])
            BW[s, c] = H.bw_adjust(control, BWmin[c], BW1[c])
            e, b = H.gammatone_bm(mid[s], BW[s, c], coscf, sincf, cfreq[c])
            ave[s, c] = np.sqrt(np.mean(e ** 2))
            cave[s, c] = np.sqrt(np.mean(control ** 2))
            g = H.compress_gain(control, attnOHC[c], lowknee[c], CR[c])
            cc, b = g * e, g * b
            sl = H.env_sl2(cc, attnIHC[c])
            b = ((sl + small) / (cc + small)) * b
            out = H.ihc_adapt(sl)
            b = ((out + small) / (sl + small)) * b
            env[s, :, c], bm[s, :, c] = out, b
    SL = np.stack([H.ave_sl(ave[s], cave[s], lossp[s][0], lossp[s][2], lossp[s][3], lossp[s][4]) for s in range(2)])
    return dict(env=env, bm=bm, sl=SL, shift=np.asarray(H.group_delay_shifts(BW[0], cfreq), dtype=np.int64), bw=BW)


def shifted(a, shift):
    """[n, 32] -> [32, n] with channel c delayed by shift[c] samples (zeros in front): what eb_EnvSmooth / eb_BMcovary are given"""
    a = np.asarray(a, dtype=np.float64)
    n = a.shape[0]
    out = np.zeros((a.shape[1], n))
    for c in range(a.shape[1]):
        s = int(shift[c])
        out[c, s:] = a[:n - s, c]
    return out


def lag_argmax(xBM, yBM):
    """The lag in [-24, 24] at which eb_BMcovary finds its maximum, for every full-window segment and band (xBM, yBM [32, n24], shifted):
    [nseg - 2, 32].  Lag l pairs x[n + l] with y[n] (np.correlate(x, y, 'full')[N - 1 + l], pyhaspi2.py:596-606)."""
    N, w = HQ_NWIN, np.hanning(HQ_NWIN)
    corr = H.window_corr(w, HQ_MAXLAG)
    lags = np.arange(-HQ_MAXLAG, HQ_MAXLAG + 1)
    nseg = n_segments(xBM.shape[1])
    out = np.zeros((nseg - 2, xBM.shape[0]), dtype=np.int64)
    for n in range(1, nseg - 1):
        sx, sy = xBM[:, n * HQ_NHALF:n * HQ_NHALF + N] * w, yBM[:, n * HQ_NHALF:n * HQ_NHALF + N] * w
        sx, sy = sx - sx.mean(axis=1, keepdims=True), sy - sy.mean(axis=1, keepdims=True)
        c = np.stack([np.sum(sx[:, max(l, 0):N + min(l, 0)] * sy[:, max(-l, 0):N - max(l, 0)], axis=1) for l in lags], axis=1)
        out[n - 1] = lags[np.argmax(np.abs(c * corr), axis=1)]
    return out


def group_spread(shift):
    """largest - smallest shift inside each group of 8 neighbouring bands (one block of hq_segment_kernel): [4]"""
    s = np.asarray(shift).reshape(4, 8)
    return s.max(axis=1) - s.min(axis=1)


def loudness_thirds(segl_c):
    """eb_3LevelCovary's histogram of the above-threshold segment loudness (pyhaspi2.py:440-472), with the distances the gate premises
    need: -> dict(bins, edges [2], margin_mid = smallest distance of a value from a mid-point between two bin centres, margin_cum =
    smallest distance of a cumulative share from 0.333 / 0.667)"""
    v = segl_c[segl_c > GATE_DB]
    bins = np.arange(np.min(v), np.max(v) + 0.5, 0.5)
    mids = (bins[:-1] + bins[1:]) / 2
    hist, _ = np.histogram(v, np.concatenate(([-1e8], (bins + np.concatenate((bins[1:], [1e8]))) / 2)))
    cum = np.cumsum(hist.astype(np.float64))
    cum = cum / cum[-1]
    edge = np.zeros(2)
    for n in range(len(bins)):
        if cum[n] < 0.333:
            edge[0] = bins[n]
        if cum[n] < 0.667:
            edge[1] = bins[n]
    mm = float(np.min(np.abs(v[:, None] - mids[None, :]))) if len(mids) else np.inf
    mc = float(min(np.min(np.abs(cum - 0.333)), np.min(np.abs(cum - 0.667))))
    return dict(bins=bins, edges=edge, margin_mid=mm, margin_cum=mc, cum=cum)


def back_end(sm, cov, msx, sl, alpha=-1.0):
    """Everything behind the segment kernel from ITS outputs (sm [2, nseg, 32], cov, msx [nseg, 32], sl [2, 32]; the oracle's functions
    take [32, nseg]) -> dict: segl [2, nseg], n_mel, n_cov, nbins, CepCorr, cov3 [3], avecov, sync5, Dloud, Dslope, Linear, Nonlin,
    Combined, Intel and the gate margins.  Where the reference raises or fails (a signal below threshold) the values are NaN, as the
    kernel reports them, with the status bits 1 (eb_melcor) and 2 (the covariance stages)."""
    nan = float('nan')
    lm, im = H._loud_index(sm[0].T, GATE_DB)
    lc, ic = H._loud_index(np.sqrt(msx).T, GATE_DB)
    o = dict(segl=np.stack([lm, lc]), n_mel=len(im), n_cov=len(ic), nbins=0, status=0, CepCorr=nan, cov3=np.full(3, nan), avecov=nan, sync5=nan)
    o['margin_seg'] = float(min(np.min(np.abs(lm - GATE_DB)), np.min(np.abs(lc - GATE_DB))))
    o['margin_cell'] = float(np.min(np.abs(np.sqrt(msx) - GATE_DB)))
    o['margin_mid'] = o['margin_cum'] = np.inf
    if len(im) > 1:
        o['CepCorr'] = H.melcor(sm[0].T, sm[1].T)[0]
    else:
        o['status'] |= 1
    if len(ic) > 1:
        th = loudness_thirds(lc)
        o.update(nbins=len(th['bins']), margin_mid=th['margin_mid'], margin_cum=th['margin_cum'], edges=th['edges'])
        o['cov3'] = H.three_level_covary(cov.T, msx.T)[0]
        avecov, syncov = H.ave_covary2(cov.T, msx.T)
        o['avecov'], o['sync5'] = float(avecov), float(syncov[4])
    else:
        o['status'] |= 2
    dloud, _dnorm, dslope = H.spect_diff(sl[0], sl[1])
    o['Dloud'] = float(np.clip(1.0 - dloud[1] / 2.5, 0, 1))
    o['Dslope'] = float(np.clip(1.0 - dslope[1], 0, 1))
    o['Linear'] = 0.579 * o['Dloud'] + 0.421 * o['Dslope']
    o['Nonlin'] = (o['CepCorr'] ** 2) * o['sync5']
    o['Combined'] = o['Nonlin'] * o['Linear']
    with np.errstate(over='ignore'):
        o['Intel'] = 1.0 / (1.0 + np.exp(alpha * (-9.047 + 14.816 * o['CepCorr'] + ((0.0 * o['cov3'][0] + 0.0 * o['cov3'][1]) + 4.616 * o['cov3'][2]))))
    return o


def oracle_stages(x, y, fs, HL=None, itype=0, r24=None):
    """Every stage of oracle/haspi.py's HASPI v1 / HASQI v2 chain on one row, named as metrics.haspi_quality_stages names them (env and bm
    before the group-delay shift), started from r24 [2, n24] float32 when given (what a kernel left as x and y at 24 kHz)."""
    r24 = normalised_r24(x, y, fs) if r24 is None else np.asarray(r24, dtype=np.float32)
    e = ear_bm(r24, HL, itype)
    sh = e['shift']
    sm = np.stack([H.env_smooth(shifted(e['env'][s], sh)).T for s in range(2)])
    cov, msx, msy = (a.T for a in H.bm_covary(shifted(e['bm'][0], sh), shifted(e['bm'][1], sh)))
    out = dict(r24=r24, shift=sh, bw=e['bw'], env=e['env'], bm=e['bm'], sl=e['sl'], sm=sm, cov=cov, msx=msx, msy=msy)
    out.update(back_end(sm, cov, msx, e['sl']))
    out['spread'] = group_spread(sh)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    x, y, fs, HL, itype = case(name)
    return oracle_stages(x, y, fs, HL, itype)


@functools.lru_cache(maxsize=None)
def ragged():
    """-> (X [6, 5000], Y, lengths, rows) at 24 kHz: one padded batch; rows[b] = (x, y) cut to the row's own length.  X and Y hold NaN
    behind each row's end."""
    Lmax = max(RAGGED_LENGTHS)
    rows = []
    for n in RAGGED_LENGTHS:
        name = {2400: 'min_2400', 2495: 'seg_2495', 2496: 'seg_2496', 2497: 'seg_2497'}.get(n)
        rows.append(case(name)[:2] if name else HC.am_pair(n, 24000, 9000 + n))
    lengths = np.array([len(r[0]) for r in rows], dtype=np.int32)
    X = np.full((len(rows), Lmax), np.nan, dtype=np.float32)
    Y = X.copy()
    for b, (x, y) in enumerate(rows):
        X[b, :len(x)], Y[b, :len(y)] = x, y
    for a in (X, Y, lengths):
        a.setflags(write=False)
    return X, Y, lengths, rows


@functools.lru_cache(maxsize=None)
def ragged_reference():
    return [oracle_stages(x, y, 24000) for (x, y) in ragged()[3]]
