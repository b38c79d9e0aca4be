"""Inputs and float64 references of the HASPI stage tests (tests/test_haspi_stages_gpu.py on the device, tests/test_haspi_cases_cpu.py for
the premises).  Plain module: numpy and oracle/haspi.py only, nothing here touches a GPU and nothing is read from a file.

A case is a pair (x clean, y = x + noise) of float32 signals: an amplitude-modulated multi-tone plus a little noise.  The lengths come
from the seams of csrc/haspi.hip (the constants below restate its #defines; test_haspi_cases_cpu.py recomputes every chunk count):
  min_2400           24 kHz, the shortest accepted signal: nsub = 267 < 615 taps of the longest modulation FIR, the fewest chunks of every kernel
  zeros_11987        24 kHz, L no multiple of 9, 16 or 32; 37 leading samples of exact zeros in x AND y (|u|^2 = 0 exactly: log2(0) in
                     the gain pass, the 1e-30 clip) and 2000 zeros inside x: 8 scan chunks, 6 middle-ear chunks, kept frames that are not
                     contiguous, more than MS_TC = 1024 ACTIVE frames (two chunks of the modulation kernel)
  seam_3071/2/3      24 kHz, one short of / on / one past two scan chunks of 1536: a third chunk that holds ONE sample (3073)
  rs16k_9001         16 kHz, odd L: haspi_resample3_kernel, 18 chunks of RS_CH = 768 outputs, librosa's zero-padded last sample
  rs22k_10000, rs8k_5000   the generic haspi_resample_kernel; a ratio of 3
  lowband_6000       24 kHz, tones <= 600 Hz and NO noise in x: control level below 50 dB in the high channels (BW = BWmin exactly)
  hl_mild_4801       24 kHz with the audiogram HL_MILD: haspi_loss_kernel's table, BWmin > 1 for y, attnIHC
  dither_4803        24 kHz with dither rows (oracle.haspi.dither_rows): row k perturbs the k-th ACTIVE frame, x and y rows apart
and ragged(): six rows of different lengths in one padded call, NaN behind every row's end."""
import functools

import numpy as np

from oracle import haspi as H

# csrc/haspi.hip
GS_LC, GS_RC, ME_N, GL_N, RS_CH, CP_F, MS_TC, MS_R, HP_SPACE, MAXFIR = 1536, 16, 2048, 2048, 768, 128, 1024, 640, 9, 615
HL_MILD = (20.0, 20.0, 25.0, 30.0, 40.0, 45.0)          # tests/golden/make_golden_haspi.py, tests/test_haspi_quality_gpu.py
DITHER_ID, DITHER_SEED = 424242, 11
GATE_DB = 2.5


def env_budget_db():
    """A-priori worst case, in dB, of the float32 arithmetic between the stored |u|^2 values and the stored dB-SL envelope
    (haspi_bank_scan_kernel<true,true,false,true>): env = s_off + T log2(g g e) with T = float32(10 log10 2), e = float32 |u|^2, g = float32
    low-passed gain, gain = exp2(K (-attn - slope (le - knee))), le = c_off + T log2(ctl).  u = 2^-24 is half a float32 ulp, relative;
    a relative error r of a power is 10 / ln 10 r dB; v_log_f32 / v_exp_f32 are accurate to 1 ulp (AMD CDNA ISA guide)."""
    u, T, K = 2.0 ** -24, 10 * np.log10(2.0), np.log2(10.0) / 20
    dbu = 10 / np.log(10.0) * u
    t_rep = abs(float(np.float32(T)) - T) * 64               # T's own rounding times |log2| < 64 (gain^2 |u|^2 spans 2^-10 .. 2^56)
    log_ulp = 2.0 ** -18 * T                                  # one ulp of a log2 result in [32, 64)
    # the dB-SL conversion: roundings of e, g, g g, (g g) e = 5 u on the argument; the log; the product T log2 (< 256: half an ulp is
    # 2^-17); s_off (< 128) and the sum (< 64)
    sl = 5 * dbu + log_ulp + 2.0 ** -17 + t_rep + 2.0 ** -18 + 2.0 ** -19
    # the control level le (< 128), likewise from one rounded |u|^2
    le = dbu + log_ulp + 2.0 ** -17 + t_rep + 2.0 ** -18 + 2.0 ** -18
    # the gain in dB: slope <= 1 - 1 / 3.5 on le and on the rounding of (le - knee); two roundings below 64 dB; the exponent K (...) < 16
    # (half an ulp 2^-21, 20 log10 2 dB each); K's own rounding on at most 70 dB; exp2 to one ulp and the float32 gain (4 u of an amplitude);
    # the low-pass of the gain is a positive filter of unit DC gain and does not enlarge an error bound
    k_rep = abs(float(np.float32(K)) - K) / K * 70
    gain = (1 - 1 / 3.5) * (le + 2.0 ** -18) + 2 * 2.0 ** -19 + 2.0 ** -21 * 20 * np.log10(2.0) + k_rep + 4 * dbu
    return sl + gain


ENV_DB = env_budget_db()        # 6.0e-5 dB
LP_DB = 2 * ENV_DB + 2.0 ** -18  # 1.24e-4 dB: the IHC adaptation's output gain R1inv = 2, the float32 rounding of its output (< 128), a unit-sum window
# name -> (fs, L, n24, nsub, n_active, smallest shift, largest shift, channels of x with BW = BWmin exactly)
EXPECTED = {
    'min_2400': (24000, 2400, 2400, 267, 256, 0, 433, 12),
    'zeros_11987': (24000, 11987, 11987, 1332, 1178, 0, 433, 12),
    'seam_3071': (24000, 3071, 3071, 342, 331, 0, 433, 12),
    'seam_3072': (24000, 3072, 3072, 342, 327, 0, 433, 12),
    'seam_3073': (24000, 3073, 3073, 342, 332, 0, 433, 12),
    'rs16k_9001': (16000, 9001, 13502, 1501, 1488, 0, 433, 12),
    'rs22k_10000': (22050, 10000, 10885, 1210, 1196, 0, 433, 12),
    'rs8k_5000': (8000, 5000, 15000, 1667, 1657, 0, 433, 16),
    'lowband_6000': (24000, 6000, 6000, 667, 657, 0, 433, 24),
    'hl_mild_4801': (24000, 4801, 4801, 534, 523, 0, 433, 12),
    'dither_4803': (24000, 4803, 4803, 534, 521, 0, 433, 12),
}
ZERO_HEAD, ZERO_GAP = 37, (5000, 7000)
RAGGED_LENGTHS = (5000, 2400, 4006, 3073, 4641, 3072)           # 4006 % 9 == 1, 4641 % 32 == 1, 5000 = the padded length


def dims(L, fs):
    """-> (n24, nsub): samples at 24 kHz (librosa: ceil(L * ratio)) and sub-sampled frames of an L-sample signal at fs"""
    n24 = L if fs == 24000 else int(np.ceil(L * (24000.0 / fs)))
    return n24, -(-n24 // HP_SPACE)


def am_pair(L, fs, seed, tones=(170.0, 410.0, 930.0, 1870.0, 3100.0, 5200.0), noise=0.02, snr_noise=0.25):
    """x: tones (those below 0.45 fs) under a 6 Hz + 31 Hz amplitude modulation, plus white noise; y = x + white noise"""
    rng = np.random.default_rng(seed)
    t = np.arange(L) / float(fs)
    x = np.zeros(L)
    for k, f in enumerate(f for f in tones if f < 0.45 * fs):
        x += (0.3 / (1 + 0.3 * k)) * np.sin(2 * np.pi * f * t + rng.uniform(0, 2 * np.pi))
    x *= 1.0 + 0.6 * np.sin(2 * np.pi * 6.0 * t + 0.3) + 0.3 * np.sin(2 * np.pi * 31.0 * t + 1.1)
    x += noise * rng.standard_normal(L)
    y = x + snr_noise * rng.standard_normal(L)
    return x.astype(np.float32), y.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (x, y, fs, HL or None, dither [2, nsub, 32] or None)"""
    fs, L = EXPECTED[name][:2]
    HL = dither = None
    if name == 'lowband_6000':
        x, y = am_pair(L, fs, 77, tones=(150.0, 260.0, 410.0, 600.0), noise=0.0, snr_noise=0.002)
    else:
        x, y = am_pair(L, fs, 5000 + L)
    if name == 'zeros_11987':
        x[:ZERO_HEAD] = 0.0
        y[:ZERO_HEAD] = 0.0
        x[ZERO_GAP[0]:ZERO_GAP[1]] = 0.0
    if name == 'hl_mild_4801':
        HL = HL_MILD
    if name == 'dither_4803':
        dither = H.dither_rows(DITHER_ID, DITHER_SEED, dims(L, fs)[1])
        dither.setflags(write=False)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y, fs, HL, dither


def oracle_stages(x, y, fs, HL=None, dither=None, r24=None):
    """Every stage of oracle/haspi.py on one row (float64 unless noted), named as metrics.haspi_stages names them:
      r24 [2, n24] float32 (the reference's own resampler accumulates in float32), mid [2, n24], ctl [2, n24, 32] control |u|^2 without the
      filter gain, bw [2, 32], bwmin [2, 32], shift [32] int, env [2, n24, 32] dB SL before IHC adaptation, lp [2, nsub, 32], gate [nsub]
      (the silence gate's level per frame in dB), index [n_active], n_active, cep [2, 6, n_active], xf [n_active, 50], yf, cm [5, 10], loss
      [2, 5, 32], raw (float) and margin = the smallest distance in dB of any frame's gate level from 2.5 dB.
    The chain is haspi_v2's own (pyhaspi2.py:76-107), restated so that it can start behind the resampler: with r24 [2, n24] (float32: what a
    kernel left as x and y at 24 kHz) the stages from the middle ear on are those of THAT input - the float32 roundings of the
    resampler, which the reference has too, stay out of the float64 comparisons.  test_haspi_cases_cpu.py checks raw against haspi_v2.
    dither [2, nsub, 32]: row k of each half perturbs the k-th active frame."""
    if r24 is None:
        x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
        L = min(len(x), len(y))
        x, y = x[:L], y[:L]
        x = x / np.sqrt(np.sum(x ** 2) / L)
        y = y / np.sqrt(np.sum(y ** 2) / L)
        r24 = np.stack([H.resample_24k(x, fs), H.resample_24k(y, fs)]).astype(np.float32)
    else:
        r24 = np.asarray(r24, dtype=np.float32)
    xdB, ydB, p = H.ear_model(r24[0], H.FSAMP, r24[1], H.FSAMP, HL=HL, itype=0)
    xLP, yLP = H.env_filt(xdB, ydB)
    with np.errstate(divide='ignore'):
        gate = 20 * np.log10(np.sum(np.power(10, xLP / 20), axis=1) / H.NCHAN)
    na = int(np.sum(gate > GATE_DB))
    dx, dy = (None, None) if dither is None else (dither[0, :na], dither[1, :na])
    xcep, ycep, index = H.cep_coef(xLP, yLP, dither_x=dx, dither_y=dy)
    assert np.array_equal(np.where(gate > GATE_DB)[0], index)
    xmod, ymod = H.mod_filt(xcep, ycep)
    aveCM, CM = H.mod_corr(xmod, ymod, full=True)
    raw = float(np.sum(H.WEIGHTS * aveCM))
    cfreq = p['cfreq']
    g1 = np.array([H.gammatone_coeffs(p['BW1'][n], cfreq[n])[6] for n in range(H.NCHAN)])
    lossx, lossy = H._loss_pair(HL, 0)
    xf = np.stack([xmod[j][m] for j in range(1, 6) for m in range(10)], axis=1)
    yf = np.stack([ymod[j][m] for j in range(1, 6) for m in range(10)], axis=1)
    return dict(r24=r24, mid=np.stack([p['xmid'], p['ymid']]),
                ctl=np.stack([np.square(p['xctl'] / g1[:, None]).T, np.square(p['yctl'] / g1[:, None]).T]),
                bw=np.stack([p['BWx'], p['BWy']]), bwmin=np.stack([lossx[1], lossy[1]]), shift=np.asarray(p['shifts'], dtype=np.int64),
                env=np.stack([p['xsl'].T, p['ysl'].T]), lp=np.stack([xLP, yLP]), gate=gate, index=np.asarray(index),
                n_active=na, cep=np.stack([xcep.T, ycep.T]), xf=xf, yf=yf, cm=CM[1:6].copy(),
                loss=np.stack([np.stack(lossx), np.stack(lossy)]), raw=raw, margin=float(np.min(np.abs(gate - GATE_DB))))


@functools.lru_cache(maxsize=None)
def reference(name):
    return oracle_stages(*case(name))


@functools.lru_cache(maxsize=None)
def ragged():
    """-> (X [6, 5000], Y, lengths, rows) at 24 kHz: one padded batch; rows[b] = (x, y) cut to the row's own length.  X and Y hold NaN
    behind each row's end."""
    Lmax = max(RAGGED_LENGTHS)
    rows = []
    for n in RAGGED_LENGTHS:
        name = {2400: 'min_2400', 3072: 'seam_3072', 3073: 'seam_3073'}.get(n)
        rows.append(case(name)[:2] if name else am_pair(n, 24000, 9000 + n))
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
