"""The clock-drift compensator of DESIGN.md section 19 restated in float64 numpy, one stream at a time: the fractional, moving delay
line on a 65 x 64 table of Kaiser-windowed sincs and the second-order loop on the phase slope between a fast and a slow average of
the SCOT-weighted cross-spectrum.  Written from that section, not from csrc/drift.hip; tests/test_drift_cpu.py checks it on its own,
tests/test_drift_gpu.py holds the kernel to it (on the library's table, which DriftRef takes as an argument)."""
import numpy as np

HOP, NFFT, NBINS = 256, 512, 257
PHASES, TAPS, BETA, SMOOTH, EPS, TINY, WARM, MAX_RATE = 64, 64, 8.0, 0.9, 1e-6, 1e-12, 32, 1e-3
TAU_MIN = 31.0


def table():
    """T[p][k], p = 0 .. 64, k = 0 .. 63: t = k - 31 - p / 64, sinc(t) I0(beta sqrt(max(0, 1 - (t / 32)^2))) / I0(beta).  sin(pi t) is
    taken on t less its nearest integer (exact) so that a whole t gives an exact zero: row 64 is row 0 moved by one tap, bit for bit."""
    p, k = np.arange(PHASES + 1)[:, None], np.arange(TAPS)[None, :]
    t = (k - 31.0) - p / float(PHASES)
    near = np.round(t)
    s = np.sin(np.pi * (t - near)) * np.where(near % 2 == 0, 1.0, -1.0)
    sinc = np.where(t == 0.0, 1.0, s / (np.pi * np.where(t == 0.0, 1.0, t)))
    return sinc * np.i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - (t / 32.0) ** 2))) / np.i0(BETA)


def tau_max(blocks):
    return float(HOP * (blocks + 3) - 33)


class DriftRef:
    def __init__(self, blocks, taps=None, lam_fast=0.9, lam_slow=0.99, kp=0.02, ki=5e-4):
        self.Q, self.R = int(blocks), int(blocks) + 4
        self.T = table() if taps is None else np.asarray(taps, dtype=np.float64).reshape(PHASES + 1, TAPS)
        self.lam_fast, self.lam_slow, self.kp, self.ki = float(lam_fast), float(lam_slow), float(kp), float(ki)
        self.tau_max = tau_max(self.Q)
        self.hist = np.zeros(self.R * HOP)                 # the ring: the last R hops of `played`, the newest sample last
        self.tau, self.rate, self.base, self.snaps = 0.0, 0.0, -1, 0
        self._clear()
        self.lowest_read = self.R * HOP                    # the oldest ring position a hop has read (0 = the ring's oldest sample)
        self.highest_read = -1

    def _clear(self):
        self.n, self.delta = 0, 0.0
        self.u_prev = np.zeros(HOP)
        self.S_d, self.S_u = np.zeros(NBINS), np.zeros(NBINS)
        self.C_f, self.C_s = np.zeros(NBINS, dtype=np.complex128), np.zeros(NBINS, dtype=np.complex128)

    @property
    def drift_ppm(self):
        return -1e6 * self.rate

    def set_rate(self, rate):
        if abs(rate) <= MAX_RATE:
            self.rate = float(rate)

    def begin_call(self, base):
        """what a call does before its first hop with base_hops[slot] -> whether the slot snapped"""
        if not (0 <= base < self.Q) or base == self.base:
            return False
        self.tau, self.base = max(float(HOP * base), TAU_MIN), int(base)
        self.snaps += 1
        self._clear()
        return True

    def hop(self, d, x, adapt=True):
        """mic d [256], played x [256] (the kernel's are float32, promoted exactly) -> aligned float32 [256]"""
        d, x = np.asarray(d, dtype=np.float64), np.asarray(x, dtype=np.float64)
        self.hist = np.concatenate([self.hist[HOP:], x])
        if self.base < 0:
            return np.zeros(HOP, dtype=np.float32)
        j = np.arange(HOP)
        t = np.clip(self.tau + self.rate * (j + 1.0), TAU_MIN, self.tau_max)
        q = (t - 31.0) * 64.0
        qi = np.floor(q)
        a = q - qi
        qi = qi.astype(np.int64)
        D, p = qi // PHASES, qi % PHASES
        at = (self.R - 1) * HOP + j - D                    # where tap 0 of sample j reads
        self.lowest_read, self.highest_read = min(self.lowest_read, int(at.min()) - (TAPS - 1)), max(self.highest_read, int(at.max()))
        acc = np.zeros(HOP)
        T0, T1 = self.T[p], self.T[p + 1]
        for k in range(TAPS):
            acc = acc + (T0[:, k] + a * (T1[:, k] - T0[:, k])) * self.hist[at - k]
        u32 = acc.astype(np.float32)
        u = u32.astype(np.float64)
        self.tau = min(max(self.tau + 256.0 * self.rate, TAU_MIN), self.tau_max)
        U = np.fft.rfft(np.concatenate([self.u_prev, u]))
        Dm = np.fft.rfft(np.concatenate([np.zeros(HOP), d]))
        self.u_prev = u
        self.S_d = SMOOTH * self.S_d + (1.0 - SMOOTH) * (Dm.real ** 2 + Dm.imag ** 2)
        self.S_u = SMOOTH * self.S_u + (1.0 - SMOOTH) * (U.real ** 2 + U.imag ** 2)
        c = Dm * np.conj(U) / np.sqrt(self.S_d * self.S_u + EPS)
        self.C_f = self.lam_fast * self.C_f + (1.0 - self.lam_fast) * c
        self.C_s = self.lam_slow * self.C_s + (1.0 - self.lam_slow) * c
        self.n += 1
        z = self.C_f * np.conj(self.C_s)
        kk = np.arange(NBINS, dtype=np.float64)
        self.delta = -(512.0 / (2.0 * np.pi)) * np.sum(kk * z.imag) / (np.sum(kk * kk * np.abs(z)) + TINY)
        if self.n > WARM and adapt:
            self.rate = min(max(self.rate + self.ki * self.delta / 256.0, -MAX_RATE), MAX_RATE)
            self.tau = min(max(self.tau + self.kp * self.delta, TAU_MIN), self.tau_max)
        return u32

    def run(self, mic, played, base, adapt=True):
        """whole hops of mic / played [nh * 256] as ONE call with base_hops = base -> aligned float32 [nh * 256]"""
        self.begin_call(base)
        return np.concatenate([self.hop(mic[i:i + HOP], played[i:i + HOP], adapt) for i in range(0, len(mic) // HOP * HOP, HOP)])
