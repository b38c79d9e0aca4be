"""Float64 reference of the SII-optimal band gains, written from the arithmetic contract of DESIGN.md section 22 (not from the kernels):
numpy, one frame at a time.  tests/siiopt_cases.py builds the scenarios on it; tests/test_siiopt_cpu.py checks its optimality and its
figures; tests/test_siiopt_gpu.py holds the kernels to it.

    P = float64(cb) ** 6 (as x2 = x x, x2 x2 x2);  N = max(float64(nb) ** 6, NMIN), a NaN giving NMIN
    Sbar += max(1 / (t + 1), 1 - lam) (P - Sbar)
    water-filling at r = sum Sbar over {gamma > 0 and Sbar > 0};  alpha = p / Sbar (1 where Sbar = 0), clamped to exp(-+LOGMAX)
    mask = float32(alpha) if strength == 1 else float32(exp(strength log alpha))
"""
import numpy as np

LAMBDA = 0.98
NMIN = 1e-30
LOGMAX = 3.2
NB = 64
GMTBAND = [0, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 28, 30, 32, 34,
           36, 38, 41, 43, 46, 49, 52, 55, 58, 62, 66, 70, 74, 79, 83, 88, 93, 99, 105, 111, 117, 124, 131, 139, 147,
           156, 165, 174, 184, 195, 206, 218, 230, 243, 257]
CENTRES = [160, 200, 250, 315, 400, 500, 630, 800, 1000, 1250, 1600, 2000, 2500, 3150, 4000, 5000, 6300, 8000]
IMPORTANCE = [0.0083, 0.0095, 0.0150, 0.0289, 0.0440, 0.0578, 0.0653, 0.0711, 0.0818, 0.0844, 0.0882, 0.0898, 0.0868, 0.0844, 0.0771,
              0.0527, 0.0364, 0.0185]


def band_importance():
    """the contract's default gamma [64]"""
    lf = np.log(np.asarray(CENTRES, dtype=np.float64))
    dens = np.asarray(IMPORTANCE, dtype=np.float64) / (0.2316 * np.asarray(CENTRES, dtype=np.float64))
    g = np.zeros(NB)
    for i in range(NB):
        f = 31.25 * GMTBAND[i]
        width = 31.25 * (GMTBAND[min(i + 1, 63)] - GMTBAND[max(i - 1, 0)]) / 2
        if f < CENTRES[0]:
            d = 0.0
        elif f >= CENTRES[-1]:
            d = dens[-1]
        else:
            j = int(np.searchsorted(lf, np.log(f), side='right')) - 1
            w = (np.log(f) - lf[j]) / (lf[j + 1] - lf[j])
            d = (1 - w) * dens[j] + w * dens[j + 1]
        g[i] = d * width
    return g / g.sum()


def _sum(v, reverse):
    """the contract's sums: over the bands in order, or - the sensitivity experiment - in reversed order"""
    s = 0.0
    for x in (v[::-1] if reverse else v):
        s += float(x)
    return s


def waterfill(Sbar, N, gamma, reverse=False, rounds=None):
    """step 3 -> the unclamped p [64] (and, in the list ``rounds``, the number of rounds taken)"""
    Sbar, N, gamma = (np.asarray(a, dtype=np.float64) for a in (Sbar, N, gamma))
    r = _sum(Sbar, reverse)
    g = np.sqrt(gamma * N)
    act = (gamma > 0) & (Sbar > 0)
    p = np.zeros(len(Sbar))
    n = 0
    while act.any():
        n += 1
        c = (r + _sum(np.where(act, N, 0.0), reverse)) / _sum(np.where(act, g, 0.0), reverse)
        p = np.where(act, c * g - N, 0.0)
        out = act & (p <= 0)
        if not out.any():
            break
        act &= ~out
        p[out] = 0.0
    if rounds is not None:
        rounds.append(n)
    return np.where(act, p, 0.0)


def powers(cb, nb):
    """step 1 on float32 features -> P, N float64"""
    x = np.asarray(cb, dtype=np.float32).astype(np.float64)
    x2 = x * x
    P = x2 * x2 * x2
    y = np.asarray(nb, dtype=np.float32).astype(np.float64)
    y2 = y * y
    Nraw = y2 * y2 * y2
    with np.errstate(invalid='ignore'):
        N = np.where(Nraw > NMIN, Nraw, NMIN)
    return P, N


def gain(p, Sbar, strength):
    """step 4 -> float32 mask"""
    with np.errstate(divide='ignore', invalid='ignore'):
        alpha = np.where(Sbar > 0, p / np.where(Sbar > 0, Sbar, 1.0), 1.0)
    alpha = np.minimum(np.maximum(alpha, np.exp(-LOGMAX)), np.exp(LOGMAX))
    return (alpha if strength == 1 else np.exp(strength * np.log(alpha))).astype(np.float32)


def mask(cb, nb, gamma=None, lam=LAMBDA, strength=0.5, reverse=False, rounds=None):
    """cb, nb [T, 64] float32 features of one row or stream -> mask [T, 64] float32"""
    gamma = band_importance() if gamma is None else np.asarray(gamma, dtype=np.float64)
    P, N = powers(cb, nb)
    T = P.shape[0]
    out = np.empty((T, NB), dtype=np.float32)
    Sbar = np.zeros(NB)
    for t in range(T):
        k = max(1.0 / (t + 1), 1.0 - lam)
        Sbar = Sbar + k * (P[t] - Sbar)
        out[t] = gain(waterfill(Sbar, N[t], gamma, reverse, rounds), Sbar, strength)
    return out


def alpha2_utterance(m, cb):
    """the utterance-level energy normalisation of the offline chain: alpha^2 = mask sum P / sum mask P"""
    P = np.asarray(cb, dtype=np.float64) ** 6
    m = np.asarray(m, dtype=np.float64)
    return m * (P.sum() / (m * P).sum())


def alpha2_prefix(m, cb):
    """the causal form: the sums over the frames up to each frame"""
    P = np.asarray(cb, dtype=np.float64) ** 6
    m = np.asarray(m, dtype=np.float64)
    s1, s2 = np.cumsum(P.sum(axis=1)), np.cumsum((m * P).sum(axis=1))
    return m * np.where(s2 > 0, s1 / np.where(s2 > 0, s2, 1.0), 1.0)[:, None]
