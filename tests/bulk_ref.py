"""The bulk-delay search of DESIGN.md section 16 restated in float64 numpy, one stream at a time: SCOT-weighted cross-spectra of the
microphone against the last Q far-end blocks, decayed over hops, their constrained inverse transforms' energies per block, and the
hold-counted decision; then the delay line.  Written from that section, not from csrc/bulkdelay.hip; tests/test_bulk_cpu.py checks it
on its own, tests/test_bulk_gpu.py holds the kernel to it."""
import numpy as np

HOP, NFFT, NBINS, SMOOTH, EPS = 256, 512, 257, 0.9, 1e-6


class BulkRef:
    def __init__(self, blocks, lam=0.99, ratio=8.0, hold=16):
        self.Q, self.lam, self.ratio, self.hold = int(blocks), float(lam), float(ratio), int(hold)
        self.reset()

    def reset(self):
        Q = self.Q
        self.x_prev = np.zeros(HOP)
        self.X = np.zeros((Q, NBINS), dtype=np.complex128)             # X[q]: the far-end spectrum of q hops ago
        self.C = np.zeros((Q, NBINS), dtype=np.complex128)
        self.S_d, self.S_x = np.zeros(NBINS), np.zeros(NBINS)
        self.n, self.cand, self.run_len, self.delay = 0, -1, 0, -1
        self.e, self.conf = np.zeros(Q), 0.0
        self.line = np.zeros((Q, HOP), dtype=np.float32)               # line[k]: `played` of k hops ago
        self.log = []                                                   # per evaluated hop: (hops seen, q*, ok, conf, second / first, e)

    def set_delay(self, h):
        if 0 <= h < self.Q:
            self.delay = int(h)

    def hop(self, d, x):
        """mic d [256], played x [256] float32 -> aligned [256] float32"""
        x32 = np.asarray(x, dtype=np.float32)
        self.line = np.roll(self.line, 1, axis=0)
        self.line[0] = x32
        if self.delay < 0:
            self._search(np.asarray(d, dtype=np.float64), x32.astype(np.float64))
        return np.zeros(HOP, np.float32) if self.delay < 0 else self.line[self.delay].copy()

    def _search(self, d, x):
        Q = self.Q
        self.X = np.roll(self.X, 1, axis=0)
        self.X[0] = np.fft.rfft(np.concatenate([self.x_prev, x]))
        self.x_prev = x
        D = np.fft.rfft(np.concatenate([np.zeros(HOP), d]))
        self.S_d = SMOOTH * self.S_d + (1.0 - SMOOTH) * (D.real ** 2 + D.imag ** 2)
        self.S_x = SMOOTH * self.S_x + (1.0 - SMOOTH) * (self.X[0].real ** 2 + self.X[0].imag ** 2)
        Dw = D / np.sqrt(self.S_d * self.S_x + EPS)
        self.C = self.lam * self.C + Dw[None, :] * np.conj(self.X)
        self.n += 1
        if self.n < Q:
            return
        r = np.fft.irfft(self.C, NFFT, axis=1)[:, :HOP]
        e = np.sum(r * r, axis=1)
        qs = int(np.argmax(e))                                          # the lowest q with the largest e
        rest = 0.0
        for q in range(Q):
            if q != qs:
                rest += e[q]
        ok = bool(e[qs] > 0.0 and e[qs] * (Q - 1) >= self.ratio * rest)
        with np.errstate(divide='ignore', invalid='ignore'):
            self.conf = float(np.float64(e[qs] * (Q - 1)) / np.float64(rest))
        self.e = e
        second = np.max(np.delete(e, qs))
        self.log.append((self.n, qs, ok, self.conf, float(second / e[qs]) if e[qs] > 0.0 else 1.0, e))
        if ok and qs == self.cand:
            self.run_len += 1
        elif ok:
            self.cand, self.run_len = qs, 1
        else:
            self.cand, self.run_len = -1, 0
        if self.run_len >= self.hold:
            self.delay = max(qs - 1, 0)

    def run(self, mic, played):
        """whole hops of mic / played [nh * 256] -> (aligned [nh * 256] float32, lock hop or None): the lock hop is the 0-based index
        of the first aligned hop"""
        out, lock = [], None
        for m, i in enumerate(range(0, len(mic) // HOP * HOP, HOP)):
            out.append(self.hop(mic[i:i + HOP], played[i:i + HOP]))
            if lock is None and self.delay >= 0:
                lock = m
        return np.concatenate(out), lock
