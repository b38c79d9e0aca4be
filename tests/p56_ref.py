"""Host restatement of the active-speech-level contract (ITU-T P.56 method B as asl_P56.py:23-148 states it at fs = 16000, nbits = 16) in
the WINDOWED form the kernel uses (csrc/level.hip), for the tests: not the reference's text - its sample-by-sample hangover loop is
replaced by "threshold j counts sample k iff some k' in [k - 3200, k] has q[k'] >= c[j]", evaluated with numpy running maxima.

    level(x)            -> dict(counts int64 [15], sq, asl_msq, actfact, c0, status, margin_db, delta_margin_db)
    mix_gain(...)       -> the float64 gain of nele_mix_noise_var
margin_db: the smallest | |diff| - tol | over every comparison the tolerance bisection made (its result jumps when one flips);
delta_margin_db: the smallest |Delta[j] - 15.9| over the threshold decisions before it.
"""
import numpy as np

FS = 16000
NTHR = 15
HANG = 3200                                  # ceil(fs * 0.2)
MARGIN = 15.9
EPS = float(np.finfo(float).eps)
G = float(np.exp(-1.0 / (FS * 0.03)))
THRESHOLDS = 2.0 ** np.arange(-15, 0, dtype=float)
SILENT, BELOW_MARGIN, NO_CROSSING = 1, 2, 4
MIX_ZERO_NOISE, MIX_ZERO_LEVEL, MIX_BAD_ROW = 1, 2, 4


def one_pole(u):
    """y[k] = (1 - g) u[k] + z; z = g y[k], float64, in sample order (two roundings per line: Python floats never contract)."""
    b0 = 1.0 - G
    out = np.empty(len(u))
    z = 0.0
    for k, v in enumerate(u.tolist()):
        y = b0 * v + z
        z = G * y
        out[k] = y
    return out


def envelope(x):
    return one_pole(one_pole(np.abs(np.asarray(x, dtype=np.float64))))


def activity_counts(q):
    k = np.arange(len(q))
    counts = np.empty(NTHR, dtype=np.int64)
    for j, c in enumerate(THRESHOLDS):
        last = np.maximum.accumulate(np.where(q >= c, k, -1)) if len(q) else k
        counts[j] = int(np.count_nonzero((last >= 0) & (k - last <= HANG))) + 1
    return counts


def _bisect(upcount, lwcount, upthr, lwthr, margin, tol, seen):
    def near(d, t):
        seen.append(abs(abs(d) - t))
    d = upcount - upthr - margin
    near(d, tol)
    if abs(d) < tol:
        return upcount, upthr
    d = lwcount - lwthr - margin
    near(d, tol)
    if abs(d) < tol:
        return lwcount, lwthr
    midcount, midthr = (upcount + lwcount) / 2.0, (upthr + lwthr) / 2.0
    turn = 1
    while True:
        diff = midcount - midthr - margin
        near(diff, tol)
        if abs(diff) <= tol:
            return midcount, midthr
        turn += 1
        if turn > 20:
            tol = tol * 1.1
            near(diff, tol)
        if diff > tol:
            midcount, midthr = (upcount + midcount) / 2.0, (upthr + midthr) / 2.0
        elif diff < -tol:
            midcount, midthr = (midcount + lwcount) / 2.0, (midthr + lwthr) / 2.0


def level_from_counts(counts, sq, n):
    """The tail (asl_P56.py:60-94) from the counters, the sum of squares and the sample count."""
    out = {'asl_msq': 0.0, 'actfact': 0.0, 'c0': 0.0, 'status': 0, 'margin_db': float('inf'), 'delta_margin_db': float('inf')}
    a = [int(v) for v in counts]
    if a[0] == 1:
        out['status'] = SILENT
        return out
    adb = [10.0 * float(np.log10(sq / a[0] + EPS))] + [10.0 * float(np.log10(sq / (a[j] + EPS) + EPS)) for j in range(1, NTHR)]
    cdb = [20.0 * float(np.log10(c + EPS)) for c in THRESHOLDS]
    deltas = [abs(adb[0] - cdb[0] - MARGIN)]
    if adb[0] - cdb[0] < MARGIN:
        out['status'] = BELOW_MARGIN
        out['delta_margin_db'] = deltas[0]
        return out
    out['status'] = NO_CROSSING
    for j in range(1, NTHR):
        deltas.append(abs(adb[j] - cdb[j] - MARGIN))
        if adb[j] - cdb[j] <= MARGIN:
            seen = []
            ml, cl = _bisect(adb[j], adb[j - 1], cdb[j], cdb[j - 1], MARGIN, 0.5, seen)
            out['asl_msq'] = float(10.0 ** (ml / 10.0))
            out['actfact'] = (sq / n) / out['asl_msq']
            out['c0'] = float(10.0 ** (cl / 20.0))
            out['status'] = 0
            out['margin_db'] = min(seen)
            break
    out['delta_margin_db'] = min(deltas)
    return out


def level(x):
    x = np.asarray(x)
    x64 = x.astype(np.float64)
    sq = float(np.sum(x64 * x64))
    counts = activity_counts(envelope(x64))
    out = level_from_counts(counts, sq, len(x))
    out['counts'], out['sq'] = counts, sq
    return out


def mix_segment(pool_row, pool_len, offset, n):
    return np.asarray(pool_row)[(int(offset) + np.arange(n)) % int(pool_len)]


def mix_gain(segment, snr_db, speech_level):
    v = np.asarray(segment, dtype=np.float64)
    nms = float(np.mean(v * v)) if len(v) else 0.0
    if not nms > 0.0 or not speech_level > 0.0:
        return 0.0
    return float(np.sqrt(speech_level / (10.0 ** (snr_db / 10.0) * nms)))
