"""The stream converter's specification restated in numpy float64, one stream at a time.  Not the product path:
tests compare the library's host functions and its GPU kernel against this file, and this file against resample_ref.resample of the
whole signal.  Written from the section: a history of K - 1 input samples, D = half div down, output m of the stream = y[m - D]."""
import numpy as np

import resample_ref as R

RATE, HOP = 16000, 256
PRESETS = R.PRESETS
# (sr_in, sr_out): every pair the tests run; 12 -> 16 kHz (4 / 3, D = 42) is the one with half - D down != 0
PAIRS = ((48000, 16000), (32000, 16000), (24000, 16000), (12000, 16000), (8000, 16000), (96000, 16000), (22000, 16000),
         (16000, 48000), (16000, 24000), (16000, 12000), (16000, 8000))


def ratio(sr_in, sr_out):
    g = int(np.gcd(sr_in, sr_out))
    return sr_out // g, sr_in // g


def hop_lengths(up, down, to16k):
    """(n_in, n_out) with n_in up = n_out down and 256 samples on the 16 kHz side; None when the other side is not a whole number"""
    num, den = (HOP * down, up) if to16k else (HOP * up, down)
    if num % den:
        return None
    return (num // den, HOP) if to16k else (HOP, num // den)


def delay(up, down, zeros):
    return R.half_width(up, down, zeros) // down


def record_bytes(K):
    return max(256, -(-4 * (K - 1) // 256) * 256)


def state_bytes(streams, K):
    return 256 + streams * record_bytes(K)


class StreamRef:
    """One stream through up / down with the taps h (natural order, 2 half + 1 of them), in hops of n_in -> n_out samples."""

    def __init__(self, up, down, h, n_in):
        assert (n_in * up) % down == 0
        self.up, self.down, self.n_in, self.n_out = up, down, n_in, n_in * up // down
        self.hp = R.polyphase(np.asarray(h, dtype=np.float64), up)
        self.K = self.hp.shape[1]
        self.half = (len(h) - 1) // 2
        self.D = self.half // down
        self.hist = np.zeros(self.K - 1, dtype=np.float64)           # the state: the last K - 1 input samples
        self.oldest = 0                                              # the furthest back any output has read (checked by the tests)

    def hop(self, x):
        """n_in samples -> n_out samples: output j reads x[c_rel div up - k], c_rel = (half - D down) + j down, k < K"""
        x = np.asarray(x, dtype=np.float64)
        assert x.shape == (self.n_in,)
        buf = np.concatenate([self.hist, x])
        c = (self.half - self.D * self.down) + np.arange(self.n_out) * self.down
        assert c.min() >= 0
        p, q = c % self.up, c // self.up
        assert q.max() <= self.n_in - 1                              # the newest sample an output needs is in its own hop
        idx = q[:, None] - np.arange(self.K)[None, :]                # relative to the hop's start
        assert idx.min() >= -(self.K - 1)                            # no read falls outside history + hop
        self.oldest = min(self.oldest, int(idx.min()))
        y = np.einsum('jk,jk->j', self.hp[p], buf[idx + self.K - 1])
        self.hist = buf[len(buf) - (self.K - 1):]
        return y

    def run(self, x):
        x = np.asarray(x, dtype=np.float64)
        assert len(x) % self.n_in == 0
        return np.concatenate([self.hop(x[i:i + self.n_in]) for i in range(0, len(x), self.n_in)])

    def flush(self):
        """the last D outputs: one hop of zeros, then a zero history"""
        y = self.hop(np.zeros(self.n_in))[:self.D]
        self.hist[:] = 0.0
        return y
