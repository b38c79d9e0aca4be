"""The echo canceller of DESIGN.md section 14 restated in float64 numpy, one stream at a time: the partitioned-block frequency-domain
adaptive filter (overlap-save, gradient-constrained) with the error-regularised step.  Written from that section, not from
csrc/aec.hip; tests/test_aec_cpu.py checks it on its own, tests/test_aec_gpu.py holds the kernel to it."""
import numpy as np

HOP, NFFT, NBINS, SMOOTH = 256, 512, 257, 0.9


class AecRef:
    def __init__(self, partitions, mu=0.5, gamma=4.0, delta=1e-2):
        self.P, self.mu, self.gamma, self.delta = int(partitions), float(mu), float(gamma), float(delta)
        self.x_prev = np.zeros(HOP)
        self.X = np.zeros((self.P, NBINS), dtype=np.complex128)        # X[p]: the far-end spectrum of p hops ago
        self.W = np.zeros((self.P, NBINS), dtype=np.complex128)
        self.S_e = np.zeros(NBINS)

    def hop(self, d, x, adapt=True):
        """mic d [256], played x [256] (the kernel's are float32, promoted exactly) -> (e, y) float64 [256]"""
        d, x = np.asarray(d, dtype=np.float64), np.asarray(x, dtype=np.float64)
        self.X = np.roll(self.X, 1, axis=0)
        self.X[0] = np.fft.rfft(np.concatenate([self.x_prev, x]))
        self.x_prev = x
        y = np.fft.irfft((self.W * self.X).sum(axis=0), NFFT)[HOP:]
        e = d - y
        E = np.fft.rfft(np.concatenate([np.zeros(HOP), e]))
        self.S_e = SMOOTH * self.S_e + (1.0 - SMOOTH) * (E.real ** 2 + E.imag ** 2)
        if adapt:
            D = (self.X.real ** 2 + self.X.imag ** 2).sum(axis=0) + self.gamma * self.P * self.S_e + self.delta
            G = self.mu * E / D
            g = np.fft.irfft(np.conj(self.X) * G[None, :], NFFT, axis=1)
            g[:, HOP:] = 0.0
            self.W = self.W + np.fft.rfft(g, axis=1)
        return e, y

    def run(self, mic, played, adapt=True):
        """whole hops of mic / played [nh * 256] -> (e, y) [nh * 256]"""
        out = [self.hop(mic[i:i + HOP], played[i:i + HOP], adapt) for i in range(0, len(mic) // HOP * HOP, HOP)]
        return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])

    def echo_path(self):
        """h[256 p + n] = irfft512(W_p)[n], n < 256"""
        return np.fft.irfft(self.W, NFFT, axis=1)[:, :HOP].reshape(-1)
