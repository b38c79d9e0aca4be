"""The noise suppressor of DESIGN.md section 21 restated in float64 numpy, one stream at a time: sqrt-Hann frames of the residual,
one IMCRA frame on float32(|E|^2 + eps) with the speech-presence probability left uncapped, the optimally-modified log-spectral
amplitude gain, overlap-add.  Written from that section, not from csrc/ns.hip; tests/test_ns_cpu.py checks it on its own (its tracker,
given the cap 0.9, against oracle.features.imcra_noise_psd bit for bit), tests/test_ns_gpu.py holds the kernel to it.
``apply_gains`` (section 17's: steps 1 and 5 are the same windows and overlap-add) puts a recorded gain sequence on any other signal,
so the output splits into its speech part and its noise part."""
import numpy as np

from res_ref import HOP, NBINS, NFFT, WINDOW, _Ola, apply_gains  # noqa: F401  (apply_gains is part of this module's interface)

EPS, NU_MIN = 1e-10, 1e-8
EULER = 0.5772156649015329


def exp1(x):
    """E1(x), x > 0 float64 array: below 1 the series -gamma - ln x - sum_k (-x)^k / (k k!), from 1 on the continued fraction
    e^-x / (x + 1 - 1 / (x + 3 - 4 / (x + 5 - ...))) by the modified Lentz recurrence; each element stops at its own convergence
    (a term, or a factor's distance from 1, below 2^-52), as the kernel's lanes do."""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty_like(x)
    lo = x < 1.0
    if lo.any():
        xs = x[lo]
        ans, fact = -np.log(xs) - EULER, np.ones_like(xs)
        live = np.ones(xs.shape, dtype=bool)
        for i in range(1, 41):
            fact = fact * (-xs / i)
            d = -fact / i
            ans = np.where(live, ans + d, ans)
            live = live & ~(np.abs(d) < np.abs(ans) * 2.0 ** -52)
            if not live.any():
                break
        out[lo] = ans
    if (~lo).any():
        xs = x[~lo]
        b = xs + 1.0
        c = np.full_like(xs, 1e300)
        d = 1.0 / b
        h = d.copy()
        live = np.ones(xs.shape, dtype=bool)
        for i in range(1, 201):
            an = -float(i) * i
            b = b + 2.0
            d = 1.0 / (an * d + b)
            c = b + an / c
            t = c * d
            h = np.where(live, h * t, h)
            live = live & ~(np.abs(t - 1.0) < 2.0 ** -52)
            if not live.any():
                break
        out[~lo] = h * np.exp(-xs)
    return out


def _fsmooth(P):
    """three taps [1/4, 1/2, 1/4], the edge rows [2/3, 1/3] / [1/3, 2/3]; float64, summed left to right"""
    P = P.astype(np.float64)
    K = P.shape[0]
    w = np.tile(np.array([0.5, 1.0, 0.5]), (K, 1))
    w[0, 0] = 0.0
    w[K - 1, 2] = 0.0
    w = w / np.sum(w, 1, keepdims=True)
    Pm = np.concatenate((P[:1], P[:-1]))
    Pp = np.concatenate((P[1:], P[-1:]))
    return (w[:, 0] * Pm + w[:, 1] * P) + w[:, 2] * Pp


class ImcraTracker:
    """Section 21 step 3: one IMCRA frame per call on Y2f (float32 [257]), the steps, constants and float32 staging of the
    project's IMCRA (csrc/imcra.h).  p_cap: 1.0 is section 21 (uncapped), 0.9 the enhancer's tracker."""

    def __init__(self, p_cap=1.0):
        self.p_cap = p_cap
        self.l = self.j = self.u = 0
        self.Storing, self.tStoring = np.zeros((NBINS, 8)), np.zeros((NBINS, 8))

    def frame(self, Y2):
        """-> (xi, Gamma, p, lambda_D after the frame, (I, q) - None before frame 15)"""
        assert Y2.dtype == np.float32 and Y2.shape == (NBINS,)
        IS, U, V = 15, 8, 15
        alpha_s, alpha_d = 0.9, 0.85
        Gamma0, Gamma1, zeta0, beta, Bmin = 4.6, 3, 1.67, 1.47, 3.2
        alpha_dd, xi_min = 0.92, 10 ** (-25. / 20)
        l = self.l
        if l == 0:
            self.G, self.Gamma, self.Lambda_D = 1, 1, 1e-6 * np.ones(NBINS)
        xi_G = (self.G ** 2) * self.Gamma
        Gamma = Y2 / self.Lambda_D                       # float32 in frames 1..15, where Lambda_D is
        xi_ML = Gamma - 1
        xi_ML[xi_ML < 1e-6] = 1e-6
        xi = alpha_dd * xi_G + (1 - alpha_dd) * xi_ML
        xi = np.asarray(xi, dtype=np.float64)
        xi[xi < xi_min] = xi_min
        self.G, self.Gamma = xi / (1 + xi), Gamma
        Sf = _fsmooth(Y2)
        if l == 0:
            self.S = Sf
            self.tS, self.Smin, self.tSmin, self.Smin_sw, self.tSmin_sw = Sf.copy(), Sf.copy(), Sf.copy(), Sf.copy(), Sf.copy()
            self.ovL = Y2
            self.Lambda_D = Y2
        self.S = alpha_s * self.S + (1 - alpha_s) * Sf
        self.Smin = np.minimum(self.Smin, self.S)
        self.Smin_sw = np.minimum(self.Smin_sw, self.S)
        p, dec = np.zeros(NBINS), None
        if l < IS:
            self.Lambda_D = alpha_d * self.Lambda_D + (1 - alpha_d) * Y2          # float32
        else:
            S = self.S
            Gamma_min = Y2 / (Bmin * self.Smin)
            zeta = S / (Bmin * self.Smin)
            I = np.zeros(NBINS)
            I[(Gamma_min < Gamma0) & (zeta < zeta0)] = 1
            norm = _fsmooth(I)
            tSf = _fsmooth(I * Y2)
            pos = norm > 0
            tSf[pos] = tSf[pos] / norm[pos]
            self.tS = alpha_s * self.tS + (1 - alpha_s) * tSf
            self.tSmin = np.minimum(self.tSmin, self.tS)
            self.tSmin_sw = np.minimum(self.tSmin_sw, self.tS)
            tGamma_min = Y2 / (Bmin * self.tSmin)
            tzeta = S / (Bmin * self.tSmin)
            q = np.zeros(NBINS)
            q[(tGamma_min <= 1) & (tzeta < zeta0)] = 1
            m = (1 < tGamma_min) & (tGamma_min < Gamma1) & (tzeta < zeta0)
            q[m] = (Gamma1 - tGamma_min[m]) / (Gamma1 - 1)
            nu = Gamma * xi / (1 + xi)
            a = q < 1
            p[a] = 1. / (1 + (q[a] / (1 - q[a])) * (1 + xi[a]) * np.exp(-nu[a]))
            p[p > self.p_cap] = self.p_cap
            tad = alpha_d + (1 - alpha_d) * p
            self.ovL = tad * self.ovL + (1 - tad) * Y2
            self.Lambda_D = beta * self.ovL
            dec = (I, q)
            self.j += 1
            if self.j == V:
                self.Storing[:, self.u % U] = self.Smin_sw                        # np.roll of the U columns == a ring
                self.tStoring[:, self.u % U] = self.tSmin_sw
                n = min(self.u + 1, U)
                self.Smin = np.min(self.Storing[:, :n], 1)
                self.Smin_sw = self.S
                self.tSmin = np.min(self.tStoring[:, :n], 1)
                self.tSmin_sw = self.tS
                self.j = 0
                self.u += 1
        self.l += 1
        return xi, Gamma, p, self.Lambda_D, dec


class NsRef:
    """y2_hook: Y2f -> Y2f (float32), applied between steps 2 and 3 - the sensitivity experiment's handle; None: section 21"""

    def __init__(self, gmin=0.1, y2_hook=None):
        self.gmin, self.y2_hook = float(gmin), y2_hook
        self.x_prev = np.zeros(HOP)
        self.tracker = ImcraTracker()
        self.ola = _Ola()

    def hop(self, x):
        """residual x [256] (the kernel's is float32, promoted exactly) -> dict: out float32 [256] (the suppressed PREVIOUS hop),
        gains, noise_psd, presence float64 [257], Y2f, and dec = (I, q) from frame 15 on"""
        x = np.asarray(x, dtype=np.float64)
        E = np.fft.rfft(WINDOW * np.concatenate([self.x_prev, x]))
        self.x_prev = x
        Y2f = (E.real ** 2 + E.imag ** 2 + EPS).astype(np.float32)
        if self.y2_hook is not None:
            Y2f = self.y2_hook(Y2f)
        xi, Gamma, p, lam, dec = self.tracker.frame(Y2f)
        nu = Gamma * xi / (1 + xi)
        G_H1 = np.minimum(xi / (1 + xi) * np.exp(0.5 * exp1(np.maximum(nu, NU_MIN))), 1.0)
        G = np.exp(p * np.log(G_H1) + (1 - p) * np.log(self.gmin))
        return {'out': self.ola.hop(G * E), 'gains': G, 'noise_psd': lam.astype(np.float64), 'presence': p, 'Y2f': Y2f, 'dec': dec}

    def run(self, x):
        """whole hops of x [nh * 256] -> dict: out float32 [nh * 256]; gains, noise_psd, presence [nh, 257]; I, q [nh, 257] (NaN
        before frame 15)"""
        hops = [self.hop(x[i:i + HOP]) for i in range(0, len(x) // HOP * HOP, HOP)]
        r = {'out': np.concatenate([h['out'] for h in hops])}
        for k in ('gains', 'noise_psd', 'presence', 'Y2f'):
            r[k] = np.stack([h[k] for h in hops])
        nan = np.full(NBINS, np.nan)
        r['I'] = np.stack([nan if h['dec'] is None else h['dec'][0] for h in hops])
        r['q'] = np.stack([nan if h['dec'] is None else h['dec'][1] for h in hops])
        return r
