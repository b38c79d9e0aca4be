"""The scheduled stream converter's specification restated in numpy float64, one stream at a time.  Not the product
path: tests compare the library's host functions and its GPU kernel against this file, and this file against resample_ref.resample of
the whole signal.  Written from the section: the 16 kHz side moves 256 samples per hop, the other side floor((g + 1) r) - floor(g r) at
schedule position g; a slot is H = K - 1 + E input samples of history and its lead L; output m of the stream = y[m - D]."""
from fractions import Fraction

import numpy as np

import resample_ref as R

RATE, HOP = 16000, 256
PRESETS = R.PRESETS
FAMILY = ((44100, 16000), (22050, 16000), (11025, 16000), (88200, 16000), (16000, 44100), (16000, 22050), (16000, 11025))
WHOLE = ((48000, 16000), (12000, 16000), (16000, 48000))            # P = 1: section 15's converter
PAIRS = FAMILY + WHOLE


def ratio(sr_in, sr_out):
    g = int(np.gcd(sr_in, sr_out))
    return sr_out // g, sr_in // g


def plan(up, down, zeros, to16k):
    """-> dict(K, D, L0, E, H, r, P, W, hop_min, hop_max) of section 20; r a Fraction, device-side samples per hop"""
    half = R.half_width(up, down, zeros)
    K = R.table_width(up, down, zeros)
    r = Fraction(HOP * down, up) if to16k else Fraction(HOP * up, down)
    P = r.denominator
    side = up if to16k else down                                     # the lead moves in steps of side / P
    assert side % P == 0
    W = side - side // P
    D = (half + W) // down
    L0 = half - D * down
    E = max(0, -((L0 - W) // up))                                    # ceil((W - L0) / up)
    return {'K': K, 'D': D, 'L0': L0, 'E': E, 'H': K - 1 + E, 'r': r, 'P': P, 'W': W, 'hop_min': int(r), 'hop_max': -int(-r // 1)}


def widths(up, down, to16k, pos, nh):
    """(n_in, n_out) of a call of nh hops from schedule position pos"""
    r = Fraction(HOP * down, up) if to16k else Fraction(HOP * up, down)
    dev = int((pos + nh) * r) - int(pos * r)                         # floor: the operands are not negative
    return (dev, nh * HOP) if to16k else (nh * HOP, dev)


def record_bytes(H):
    return -(-(16 + 4 * H) // 256) * 256


def state_bytes(streams, H):
    return 256 + streams * record_bytes(H)


class SchedRef:
    """One stream through up / down with the taps h (natural order, 2 half + 1 of them), from schedule position pos"""

    def __init__(self, up, down, h, to16k, pos=0):
        self.up, self.down, self.to16k = up, down, bool(to16k)
        self.hp = R.polyphase(np.asarray(h, dtype=np.float64), up)
        self.K = self.hp.shape[1]
        self.half = (len(h) - 1) // 2
        assert self.half % max(up, down) == 0
        p = plan(up, down, self.half // max(up, down), to16k)
        assert p['K'] == self.K
        self.D, self.L0, self.E, self.H, self.P, self.W = p['D'], p['L0'], p['E'], p['H'], p['P'], p['W']
        self.pos = pos
        self.reset(pos)

    def reset(self, pos):
        assert 0 <= pos < self.P
        self.pos, self.L = pos, self.L0
        self.hist = np.zeros(self.H, dtype=np.float64)
        self.oldest, self.leads = 0, [self.L0]

    def in_bounds(self, n_in, n_out, L=None):
        """the device's guard: would a call of these widths read inside history + row from the lead L?"""
        L = self.L if L is None else L
        return L >= -self.E * self.up and L + (n_out - 1) * self.down < n_in * self.up

    def hop(self, x):
        """the hop at the stream's position: output j reads x[c_rel div up - k], c_rel = L + j down, k < K (floor division)"""
        x = np.asarray(x, dtype=np.float64)
        n_in, n_out = widths(self.up, self.down, self.to16k, self.pos, 1)
        assert x.shape == (n_in,)
        buf = np.concatenate([self.hist, x])
        c = self.L + np.arange(n_out) * self.down
        p, q = c % self.up, c // self.up                             # numpy: floor division, a remainder that is not negative
        assert q.max() <= n_in - 1                                   # the newest sample an output needs is in its own hop
        idx = q[:, None] - np.arange(self.K)[None, :]                # relative to the hop's start
        assert idx.min() >= -self.H                                  # no read falls outside history + hop
        self.oldest = min(self.oldest, int(idx.min()))
        y = np.einsum('jk,jk->j', self.hp[p], buf[idx + self.H])
        self.hist = buf[len(buf) - self.H:]
        self.L += n_out * self.down - n_in * self.up
        assert self.L < self.down                                    # behind every hop
        assert abs(self.L - self.L0) <= self.W
        self.leads.append(self.L)
        self.pos = (self.pos + 1) % self.P
        return y

    def width_in(self, nh):
        return widths(self.up, self.down, self.to16k, self.pos, nh)[0]

    def run(self, x):
        """as many whole hops as x holds from the stream's position (x must end on a hop)"""
        x = np.asarray(x, dtype=np.float64)
        ys, i = [], 0
        while i < len(x):
            n = self.width_in(1)
            ys.append(self.hop(x[i:i + n]))
            i += n
        assert i == len(x)
        return np.concatenate(ys) if ys else np.zeros(0)

    def flush(self):
        """the last D outputs: one hop of zeros, then a reset (the position stays: the caller's bookkeeping)"""
        y = self.hop(np.zeros(self.width_in(1)))[:self.D]
        pos = self.pos
        self.reset(pos)
        return y
