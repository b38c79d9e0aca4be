"""The residual-echo suppressor of DESIGN.md section 17 restated in float64 numpy, one stream at a time: sqrt-Hann frames of the
canceller's residual e and echo estimate y, their smoothed auto- and cross-spectra, the coherence gain, overlap-add.  Written from that
section, not from csrc/res.hip; tests/test_res_cpu.py checks it on its own, tests/test_res_gpu.py holds the kernel to it.
``apply_gains`` puts a recorded gain sequence on any other signal with the same windows and overlap-add: the filter is linear in the
signal once the gains are fixed, so the output splits into its echo part and its noise part."""
import numpy as np

HOP, NFFT, NBINS, SMOOTH, EPS = 256, 512, 257, 0.9, 1e-10
WINDOW = np.sqrt(0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(NFFT) / NFFT))


class _Ola:
    """step 4: o = w irfft512(spectrum), out = float32(ola + o[0:256]), ola <- o[256:512]"""

    def __init__(self):
        self.ola = np.zeros(HOP)

    def hop(self, spec):
        o = WINDOW * np.fft.irfft(spec, NFFT)
        out = (self.ola + o[:HOP]).astype(np.float32)
        self.ola = o[HOP:].copy()
        return out


class ResRef:
    def __init__(self, beta=2.0, gmin=0.1):
        self.beta, self.gmin = float(beta), float(gmin)
        self.e_prev, self.y_prev = np.zeros(HOP), np.zeros(HOP)
        self.S_ee, self.S_yy = np.zeros(NBINS), np.zeros(NBINS)
        self.S_ey = np.zeros(NBINS, dtype=np.complex128)
        self.ola = _Ola()

    def hop(self, e, y):
        """residual e [256], echo y [256] (the kernel's are float32, promoted exactly) -> (out float32 [256], G float64 [257]);
        out is the suppressed residual of the PREVIOUS hop"""
        e, y = np.asarray(e, dtype=np.float64), np.asarray(y, dtype=np.float64)
        E = np.fft.rfft(WINDOW * np.concatenate([self.e_prev, e]))
        Y = np.fft.rfft(WINDOW * np.concatenate([self.y_prev, y]))
        self.e_prev, self.y_prev = e, y
        a = SMOOTH
        self.S_ee = a * self.S_ee + (1.0 - a) * (E.real ** 2 + E.imag ** 2)
        self.S_yy = a * self.S_yy + (1.0 - a) * (Y.real ** 2 + Y.imag ** 2)
        self.S_ey = a * self.S_ey + (1.0 - a) * (E * np.conj(Y))
        R = (self.S_ey.real ** 2 + self.S_ey.imag ** 2) / (self.S_yy + EPS)
        G = np.sqrt(np.maximum(1.0 - self.beta * R / (self.S_ee + EPS), self.gmin * self.gmin))
        return self.ola.hop(G * E), G

    def run(self, residual, echo):
        """whole hops of residual / echo [nh * 256] -> (out float32 [nh * 256], G [nh, 257])"""
        hops = [self.hop(residual[i:i + HOP], echo[i:i + HOP]) for i in range(0, len(residual) // HOP * HOP, HOP)]
        return np.concatenate([h[0] for h in hops]), np.stack([h[1] for h in hops])


def apply_gains(gains, x):
    """gains [nh, 257] as ResRef.run recorded them, x [nh * 256] any signal -> float32 [nh * 256]: what the suppressor with these gains
    makes of x (steps 1 and 4 of section 17 from zero state), one hop late like its output"""
    x = np.asarray(x, dtype=np.float64)
    prev, ola, out = np.zeros(HOP), _Ola(), []
    for h in range(len(gains)):
        cur = x[h * HOP:(h + 1) * HOP]
        out.append(ola.hop(gains[h] * np.fft.rfft(WINDOW * np.concatenate([prev, cur]))))
        prev = cur
    return np.concatenate(out)
