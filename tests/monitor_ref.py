"""The running ESTOI of DESIGN.md section 27 as a float64 numpy process: hop in, state carried - the reference of csrc/monitor.hip
(tests/test_monitor_gpu.py) and, through tests/test_monitor_cpu.py, tied to oracle/estoi.py itself.  The filter, the window and the
band matrix come from oracle/estoi.py; nothing here reads the package."""
import numpy as np

from oracle import estoi as E

HOP = 256                      # samples per hop at 16 kHz
OUT = 160                      # samples per hop at 10 kHz
BEHIND = 36                    # of them, those only the next hop can finish
HIST = 128                     # 16 kHz samples carried
NSTATS = 8
MAX_LAG = 4
COUNT, SUM, LAST, SMOOTH, SKIPPED, SEEN, KEPT, M = range(NSTATS)


def taps():
    """the 581 taps resample_poly(x, 5, 8, window=h / sum(h)) applies: unit sum, times the up factor"""
    h = E.resample_window_oct(E.FS, 16000)
    assert len(h) == 2 * 290 + 1
    return 5.0 * h / np.sum(h)


def alpha_of(time_constant):
    """the smoothing factor per segment, one segment per 12.8 ms"""
    return float(1.0 - np.exp(-0.0128 / float(time_constant)))


def final_samples(hops):
    """10 kHz samples that are final after `hops` hops: output m needs input floor((8 m + 290) / 5)"""
    n = 0
    while (8 * n + 290) // 5 <= HOP * hops - 1:
        n += 1
    return n


class Monitor:
    """One stream.  hop(ref, deg, add): 256 float32 samples each (deg, add may be None) -> the d of the segments the hop formed
    (NaN for a skipped one).  stats(): the eight readings.  frames: (en, M, kept) of every frame seen, for the tests' premises."""

    def __init__(self, lag=0, alpha=1.0):
        assert 0 <= lag <= MAX_LAG and 0.0 < alpha <= 1.0
        self.lag, self.alpha = lag, alpha
        self.h = taps()
        self.w = E.hann_sym(E.N_FRAME)
        self.obm = E.thirdoct()[0]
        # output j = -36 .. 123 of a hop: inputs lo .. hi of the hop (negative: the history), taps in the order of those inputs
        self.plan = []
        for j in range(-BEHIND, OUT - BEHIND):
            c = 8 * j + 290
            hi = c // 5
            lo = -((580 - c) // 5)                                                # the first n with c - 5 n <= 580
            self.plan.append((lo + HIST, hi + HIST + 1, self.h[c - 5 * np.arange(lo, hi + 1)]))
        self.reset()

    def reset(self):
        self.past = []                                                             # the last `lag` hops of ref
        self.started = False
        self.hist = np.zeros((2, HIST))
        self.tail = np.zeros((2, 0))
        self.first = None                                                          # [2, 128]: the next re-analysis frame's first half
        self.second = None                                                         # [2, 128]: the last kept frame's second half
        self.ring = []                                                             # the last 30 band vectors, [2, 15] each
        self.s = np.zeros(NSTATS)
        self.s[M] = -np.inf
        self.frames = []

    def stats(self):
        return self.s.copy()

    def _segment(self):
        blocks = np.stack(self.ring, axis=-1)                                      # [2, 15, 30], oldest column first
        with np.errstate(invalid='ignore', divide='ignore'):
            d = np.sum(E.row_col_normalize(blocks[0][None]) * E.row_col_normalize(blocks[1][None])) / E.N
        if np.isfinite(d):
            self.s[SMOOTH] = d if self.s[COUNT] == 0 else self.s[SMOOTH] + self.alpha * (d - self.s[SMOOTH])
            self.s[COUNT] += 1
            self.s[SUM] += d
            self.s[LAST] = d
            return float(d)
        self.s[SKIPPED] += 1
        return float('nan')

    def _kept(self, f):
        """f [2, 256]: a windowed kept frame -> the d its arrival yields, or None"""
        if self.first is None:
            self.first, self.second = f[:, :128].copy(), f[:, 128:].copy()
            return None
        mid = self.second + f[:, :128]
        spec = np.fft.rfft(self.w * np.concatenate([self.first, mid], axis=1), n=E.NFFT, axis=-1)
        with np.errstate(invalid='ignore'):
            self.ring.append(np.sqrt(np.square(np.abs(spec)) @ self.obm.T))
        self.first, self.second = mid, f[:, 128:].copy()
        self.ring = self.ring[-E.N:]
        return self._segment() if len(self.ring) == E.N else None

    def hop(self, ref, deg=None, add=None):
        ref = np.asarray(ref, dtype=np.float32)
        assert ref.shape == (HOP,)
        r = ref.astype(np.float64)
        if self.lag:
            self.past.append(r)
            if len(self.past) <= self.lag:
                return []                                                          # nothing to compare with yet
            r = self.past.pop(0)
        y = r.copy() if deg is None else np.asarray(deg, dtype=np.float32).astype(np.float64)
        if add is not None:
            y = y + np.asarray(add, dtype=np.float32).astype(np.float64)
        xin = np.concatenate([self.hist, np.stack([r, y])], axis=1)                # [2, 384]
        with np.errstate(invalid='ignore'):
            new = np.array([[np.dot(x[lo:hi], t) for (lo, hi, t) in self.plan] for x in xin])
        if not self.started:
            new = new[:, BEHIND:]                                                  # outputs before the stream's first do not exist
            self.started = True
        self.hist = xin[:, HOP:]
        self.tail = np.concatenate([self.tail, new], axis=1)
        out = []
        while self.tail.shape[1] >= E.N_FRAME:
            f = self.w * self.tail[:, :E.N_FRAME]
            self.tail = self.tail[:, E.N_FRAME // 2:]
            with np.errstate(invalid='ignore', divide='ignore'):
                en = 20 * np.log10(np.linalg.norm(f[0]) + E.EPS)
            self.s[SEEN] += 1
            if np.isfinite(en):
                self.s[M] = max(self.s[M], en)
            keep = bool(np.isfinite(en) and (self.s[M] - E.DYN_RANGE - en) < 0)
            self.frames.append((float(en), float(self.s[M]), keep))
            if keep:
                self.s[KEPT] += 1
                d = self._kept(f)
                if d is not None:
                    out.append(d)
        assert len(out) <= 2
        return out


def run(ref, deg=None, add=None, lag=0, alpha=1.0, mon=None):
    """whole signals [nh * 256] through one Monitor -> dict(seg [nh, 2] (NaN where no segment), nseg [nh], stats [8], values: the
    segments' d in order (NaN for skipped ones), frames, mon)"""
    mon = Monitor(lag, alpha) if mon is None else mon
    nh = len(ref) // HOP
    assert len(ref) == nh * HOP
    seg, nseg, values = np.full((nh, 2), np.nan), np.zeros(nh, dtype=np.int32), []
    for h in range(nh):
        cut = slice(h * HOP, (h + 1) * HOP)
        d = mon.hop(ref[cut], None if deg is None else deg[cut], None if add is None else add[cut])
        seg[h, :len(d)], nseg[h] = d, len(d)
        values += d
    return dict(seg=seg, nseg=nseg, stats=mon.stats(), values=np.array(values), frames=list(mon.frames), mon=mon)
