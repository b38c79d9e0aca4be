"""The resampler's specification restated in numpy float64, and thin wrappers around scipy.  Not the product path:
tests compare the library's host functions and its GPU kernel against this file, and this file against scipy.signal.resample_poly."""
import numpy as np

PRESETS = {'high': (32, 12.0), 'scipy': (10, 5.0)}
PAIRS = ((1, 3), (2, 1), (3, 2), (160, 441), (640, 441), (1, 6))          # (up, down): 48 -> 16, 8 -> 16, .., 44.1 -> 16, 11.025 -> 16, 96 -> 16


def half_width(up, down, zeros):
    return zeros * max(up, down)


def table_width(up, down, zeros):
    return -(-(2 * half_width(up, down, zeros) + 1) // up)


def out_len(n_in, up, down):
    return -(-n_in * up // down)


def taps(up, down, zeros, beta):
    """h = up * h0 / sum(h0), h0[k] = fc sinc(fc (k - half)) I0(beta sqrt(1 - ((k - half) / half)^2)) / I0(beta), fc = 1 / max(up, down)"""
    half = half_width(up, down, zeros)
    fc = 1.0 / max(up, down)
    m = np.arange(-half, half + 1, dtype=np.float64)
    h0 = fc * np.sinc(fc * m) * np.i0(beta * np.sqrt(np.maximum(1.0 - (m / half) ** 2, 0.0))) / np.i0(beta)
    return up * h0 / h0.sum()


def scipy_taps(up, down, zeros, beta):
    from scipy.signal import firwin
    return up * firwin(2 * half_width(up, down, zeros) + 1, 1.0 / max(up, down), window=('kaiser', beta))


def polyphase(h, up):
    """hp[p][k] = h[p + k up], zero where p + k up is behind h's end"""
    K = -(-len(h) // up)
    hp = np.zeros((up, K), dtype=np.float64)
    for p in range(up):
        col = h[p::up]
        hp[p, :len(col)] = col
    return hp


def resample(x, up, down, h, gain=1.0, outputs=None):
    """y[n] = gain sum_k hp[p][k] x[q - k], c = n down + half, p = c mod up, q = c div up; float64.  ``outputs``: the n to evaluate
    (default: all ceil(L up / down) of them).  Python integers: no index overflows."""
    x = np.asarray(x, dtype=np.float64)
    L, half = len(x), (len(h) - 1) // 2
    hp = polyphase(np.asarray(h, dtype=np.float64), up)
    K = hp.shape[1]
    ns = range(out_len(L, up, down)) if outputs is None else outputs
    y = np.zeros(len(ns), dtype=np.float64)
    ks = np.arange(K)
    for i, n in enumerate(ns):
        c = int(n) * down + half
        p, q = c % up, c // up
        idx = q - ks
        ok = (idx >= 0) & (idx < L)
        y[i] = gain * np.dot(hp[p][ok], x[idx[ok]])
    return y


def scipy_resample(x, up, down, h):
    """scipy.signal.resample_poly on the float64 copy with the taps h (resample_poly multiplies its window by up itself)"""
    from scipy.signal import resample_poly
    x = np.asarray(x, dtype=np.float64)
    if len(x) == 0:
        return np.zeros(0, dtype=np.float64)
    return resample_poly(x, up, down, window=np.asarray(h, dtype=np.float64) / up)


def bound(y64, xmax):
    """the per-sample bound of the GPU tests: one float32 ulp of the float64 result (the summation order may move a value across a
    rounding boundary) + 1e-12 max|x| (zero crossings: K eps64 max|h| max|x| with a tenfold margin, max|h| <= 1)"""
    return np.spacing(np.abs(y64).astype(np.float32)).astype(np.float64) + 1e-12 * xmax
