"""The carried high band on a hop schedule: the specification restated in numpy float64, one stream at a time, on
schedrate_ref.SchedRef.  Not the product path: tests compare the library's host functions and its GPU kernel against this file, and
this file against the section's consequences.  Per stream, zeros before its start, lam = 256 lag_hops:

    s  = (-(D_down + lam) up) mod down                     the up-converter's slots start at the lead L0 - s instead of L0
    Lx = ((D_down + lam) up + s) / down + D_up             a whole number
    d[n] = fmaf(-g, low[n - lam], enh[n])        u = SchedRef(16 kHz -> device rate) of d from the lead L0 - s        y[m] = fmaf(g, x[m - Lx], (float)u[m])

``rounded=False`` keeps every value in float64; ``rounded=True`` rounds d, (float)u and y to float32 as the specification does
(highband_ref.fma32)."""
from fractions import Fraction

import numpy as np

import resample_ref as R
import schedrate_ref as S
from highband_ref import fma32


def plan(device_rate, lag_hops=1, quality='high', shift=None):
    """-> dict(up, down, zeros, beta, K, D_down, D_up, s, L0 (the shifted lead), E, H, W, lam, Lx, r, P, before) of the section; ``before``
    is section 20's latency (D_down + lam) up / down + D_up as a Fraction.  shift: an s to use instead of the section's (tests that show
    what the shift is for); Lx is then the next whole number at or above before + s / down."""
    zeros, beta = S.PRESETS[quality] if isinstance(quality, str) else quality
    up, down = S.ratio(S.RATE, device_rate)
    assert up > down
    pu, pd = S.plan(up, down, zeros, False), S.plan(down, up, zeros, True)
    lam = S.HOP * lag_hops
    through = (pd['D'] + lam) * up                                   # the 16 kHz side's delay in ticks of 1 / down of a device sample
    s = (-through) % down if shift is None else shift
    L0 = pu['L0'] - s
    E = max(0, -((L0 - pu['W']) // up))                              # ceil((W - L0') / up)
    Lx = Fraction(through + s, down) + pu['D']
    return {'up': up, 'down': down, 'zeros': zeros, 'beta': beta, 'K': pu['K'], 'D_down': pd['D'], 'D_up': pu['D'], 's': s, 'L0': L0, 'E': E,
            'H': pu['K'] - 1 + E, 'W': pu['W'], 'lam': lam, 'Lx': -int(-Lx // 1), 'exact': Lx.denominator == 1, 'r': pu['r'], 'P': pu['P'],
            'before': Fraction(through, down) + pu['D']}


def record_bytes(H, lam, Lx):
    return -(-(16 + 4 * (H + lam + Lx)) // 256) * 256


def state_bytes(streams, H, lam, Lx):
    return 256 + streams * record_bytes(H, lam, Lx)


def solve_ab(up, down, s):
    """the smallest integers a, b >= 0 with a down - b up = -s (gcd(up, down) = 1): the shifted converter's output m is output m + a of the
    unshifted one fed b zeros first"""
    a = (-s * pow(down, -1, up)) % up
    b = (a * down + s) // up
    assert a >= 0 and b >= 0 and a * down - b * up == -s
    return a, b


def direct(d, up, down, h, L0, count):
    """outputs 0 .. count - 1 of the stream d (zeros outside it) from the lead L0, without hops or history: c = L0 + m down, p = c mod up,
    q = c div up, sum_k hp[p][k] d[q - k] - what any grouping into calls, on or off the schedule, must give while the guard lets it run"""
    d = np.asarray(d, dtype=np.float64)
    hp = R.polyphase(np.asarray(h, dtype=np.float64), up)
    ks = np.arange(hp.shape[1])
    y = np.zeros(count)
    for m in range(count):
        c = L0 + m * down
        idx = c // up - ks
        ok = (idx >= 0) & (idx < len(d))
        y[m] = np.dot(hp[c % up][ok], d[idx[ok]])
    return y


class ShiftedSchedRef(S.SchedRef):
    """SchedRef(16 kHz -> device rate) whose slots start at the lead L0 - s: every assertion of SchedRef.hop holds with E and H
    recomputed from that lead"""

    def __init__(self, up, down, h, s, pos=0):
        super().__init__(up, down, h, False, pos)
        self.L0 -= s
        self.E = max(0, -((self.L0 - self.W) // up))
        self.H = self.K - 1 + self.E
        self.reset(pos)


class HighBandSchedRef:
    """One stream: process(enh, low, x) with nh * 256 samples of enh and low at 16 kHz and the schedule's width of nh hops of x at the
    device rate, from the stream's position -> as many samples of y."""

    def __init__(self, device_rate, lag_hops=1, quality='high', g=1.0, rounded=False, pos=0, shift=None, taps=None):
        self.__dict__.update(plan(device_rate, lag_hops, quality, shift))
        self.g, self.rounded = (np.float32(g) if rounded else float(g)), rounded
        h = R.taps(self.up, self.down, self.zeros, self.beta) if taps is None else taps
        self.upc = ShiftedSchedRef(self.up, self.down, h, self.s, pos)
        assert (self.upc.D, self.upc.L0, self.upc.E, self.upc.H) == (self.D_up, self.L0, self.E, self.H)
        self.low_hist = np.zeros(self.lam)                           # the state beside the converter's: the last lam of low, the last Lx of x
        self.x_hist = np.zeros(self.Lx)

    def width(self, nh):
        return S.widths(self.up, self.down, False, self.upc.pos, nh)[1]

    def process(self, enh, low, x):
        """nh hops in one call: the delay lines take the call's rows whole, the converter runs hop by hop"""
        enh, low, x = (np.asarray(v, dtype=np.float64) for v in (enh, low, x))
        nh = len(enh) // S.HOP
        assert nh >= 1 and enh.shape == low.shape == (nh * S.HOP,) and x.shape == (self.width(nh),)
        lows, xs = np.concatenate([self.low_hist, low]), np.concatenate([self.x_hist, x])
        low_del, x_del = lows[:len(low)], xs[:len(x)]                # low[n - lam], x[m - Lx]
        self.low_hist, self.x_hist = lows[len(low):], xs[len(x):]
        d = fma32(-self.g, low_del, enh).astype(np.float64) if self.rounded else enh - self.g * low_del
        u = np.concatenate([self.upc.hop(d[i * S.HOP:(i + 1) * S.HOP]) for i in range(nh)])
        return fma32(self.g, x_del, u.astype(np.float32)).astype(np.float64) if self.rounded else u + self.g * x_del


def path(device_rate, x, enhance, lag_hops=1, quality='high', g=1.0, groups=None, pos=0, shift=None):
    """The whole wrapper on one float64 signal x at the device rate (a whole number of hops of the schedule from ``pos``, ``groups`` of
    them per call in turn; None: one): the down-converter, ``enhance(low) -> enh`` (it owns its own lag of lam samples) and the carried
    band -> (y, plain, hb): with the band, the plain wrapper's up(enh) from the unshifted lead, and the HighBandSchedRef."""
    hb = HighBandSchedRef(device_rate, lag_hops, quality, g, pos=pos, shift=shift)
    dn = S.SchedRef(hb.down, hb.up, R.taps(hb.down, hb.up, hb.zeros, hb.beta), True, pos)
    plain = S.SchedRef(hb.up, hb.down, R.taps(hb.up, hb.down, hb.zeros, hb.beta), False, pos)
    ys, ps, at = [], [], 0
    while at < len(x):
        nh = 1 if groups is None else groups[len(ys) % len(groups)]
        xs = x[at:at + hb.width(nh)]
        low = dn.run(xs)
        enh = enhance(low)
        ys.append(hb.process(enh, low, xs))
        ps.append(plain.run(enh))
        at += len(xs)
    assert at == len(x)
    return np.concatenate(ys), np.concatenate(ps), hb
