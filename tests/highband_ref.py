"""The carried high band's specification restated in numpy float64, one stream at a time, on
streamrate_ref.StreamRef.  Not the product path: tests compare the GPU kernel against this file, and this file against the section's
consequences.  Per stream, zeros before its start, lam = 256 lag_hops, L = D_down N / 256 + lag_hops N + D_up:

    d[n] = fmaf(-g, low[n - lam], enh[n])        u = StreamRef(16 kHz -> device rate) of d        y[m] = fmaf(g, x[m - L], (float)u[m])

``rounded=False`` keeps every value in float64 (the consequences: what the arithmetic does before float32 enters); ``rounded=True``
rounds d, (float)u and y to float32 as the specification does - fma32 below is the correctly rounded float32 fused multiply-add."""
import numpy as np

import resample_ref as R
import streamrate_ref as S


def fma32(a, b, c):
    """float32 fmaf(a, b, c) of float32 operands, correctly rounded: a b is exact in float64; s = fl64(a b + c) and its error e (TwoSum)
    are exact, and rounding s to float32 differs from rounding a b + c only when s lies midway between two float32 values and e != 0 -
    then e decides.  (No overflow or subnormal results in the tests that use it.)"""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    f = s.astype(np.float32)                                         # ties to even: right when e == 0
    f64 = f.astype(np.float64)
    other = np.nextafter(f, np.where(s > f64, np.inf, -np.inf).astype(np.float32)).astype(np.float64)      # the float32 on s's other side
    tie = (s != f64) & (np.abs(s - f64) == np.abs(other - s))
    out = f64.copy()
    out[tie & (e > 0)] = np.maximum(f64, other)[tie & (e > 0)]
    out[tie & (e < 0)] = np.minimum(f64, other)[tie & (e < 0)]
    return out.astype(np.float32)


def geometry(device_rate, lag_hops=1, quality='high'):
    """-> dict(up, down, zeros, beta, N, D_down, D_up, lam, L) of the section, or None where D_down N is not a multiple of 256"""
    zeros, beta = S.PRESETS[quality] if isinstance(quality, str) else quality
    up, down = S.ratio(S.RATE, device_rate)
    N = S.hop_lengths(up, down, False)[1]
    D_down, D_up = S.delay(down, up, zeros), S.delay(up, down, zeros)
    if (D_down * N) % S.HOP:
        return None
    return {'up': up, 'down': down, 'zeros': zeros, 'beta': beta, 'N': N, 'D_down': D_down, 'D_up': D_up, 'lam': S.HOP * lag_hops,
            'L': D_down * N // S.HOP + lag_hops * N + D_up}


class HighBandRef:
    """One stream: process(enh, low, x) with nh * 256 samples of enh and low at 16 kHz and nh * N of x at the device rate -> nh * N
    samples of y."""

    def __init__(self, device_rate, lag_hops=1, quality='high', g=1.0, rounded=False):
        geo = geometry(device_rate, lag_hops, quality)
        self.__dict__.update(geo)
        self.g, self.rounded = (np.float32(g) if rounded else float(g)), rounded
        self.upc = S.StreamRef(self.up, self.down, R.taps(self.up, self.down, self.zeros, self.beta), S.HOP)
        assert self.upc.n_out == self.N and self.upc.D == self.D_up
        self.low_hist = np.zeros(self.lam)                           # the state beside the converter's: the last lam of low, the last L of x
        self.x_hist = np.zeros(self.L)

    def process(self, enh, low, x):
        """nh hops in one call: the delay lines take the call's rows whole, the converter runs hop by hop"""
        enh, low, x = (np.asarray(v, dtype=np.float64) for v in (enh, low, x))
        nh = len(enh) // S.HOP
        assert nh >= 1 and enh.shape == low.shape == (nh * S.HOP,) and x.shape == (nh * self.N,)
        lows, xs = np.concatenate([self.low_hist, low]), np.concatenate([self.x_hist, x])
        low_del, x_del = lows[:len(low)], xs[:len(x)]                # low[n - lam], x[m - L]
        self.low_hist, self.x_hist = lows[len(low):], xs[len(x):]
        d = fma32(-self.g, low_del, enh).astype(np.float64) if self.rounded else enh - self.g * low_del
        u = np.concatenate([self.upc.hop(d[i * S.HOP:(i + 1) * S.HOP]) for i in range(nh)])
        return fma32(self.g, x_del, u.astype(np.float32)).astype(np.float64) if self.rounded else u + self.g * x_del


def path(device_rate, x, enhance, lag_hops=1, quality='high', g=1.0, groups=None):
    """The whole wrapper on one float64 signal x at the device rate (a whole number of hops, ``groups`` of them per call in turn; None:
    one): the down-converter, ``enhance(low) -> enh`` (it owns its own lag of lam samples) and the carried band -> (y, plain): with the
    band, and the plain wrapper's up(enh)."""
    geo = geometry(device_rate, lag_hops, quality)
    dn = S.StreamRef(geo['down'], geo['up'], R.taps(geo['down'], geo['up'], geo['zeros'], geo['beta']), geo['N'])
    hb = HighBandRef(device_rate, lag_hops, quality, g)
    plain = S.StreamRef(geo['up'], geo['down'], R.taps(geo['up'], geo['down'], geo['zeros'], geo['beta']), S.HOP)
    N = geo['N']
    ys, ps, h = [], [], 0
    for g_ in groups or (1,) * (len(x) // N):
        xs = x[h * N:(h + g_) * N]
        low = np.concatenate([dn.hop(xs[i * N:(i + 1) * N]) for i in range(g_)])
        enh = enhance(low)
        ys.append(hb.process(enh, low, xs))
        ps += [plain.hop(enh[i * S.HOP:(i + 1) * S.HOP]) for i in range(g_)]
        h += g_
    assert h * N == len(x)
    return np.concatenate(ys), np.concatenate(ps)


class DelayedGain:
    """the stand-in enhancer: ``gain`` times its input, lam samples late"""

    def __init__(self, lam, gain):
        self.hist, self.gain = np.zeros(lam), gain

    def __call__(self, low):
        buf = np.concatenate([self.hist, low])
        self.hist = buf[len(low):]
        return self.gain * buf[:len(low)]
