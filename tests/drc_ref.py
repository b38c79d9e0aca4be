"""numpy float64 restatement of the causal dynamic range compressor of DESIGN.md section 23 (test infrastructure, like tests/ns_ref.py):
one stream, hop by hop, written from the contract - nothing of the HIP kernel's structure (ring, lanes, waves).  The taps, the curve
and the parameters are those of tests/ssdrc_ref.py (section 11)."""
import numpy as np

import ssdrc_ref as S

HOP, HIST, LOOK = 256, 400, 144
TAU_PEAK, TAU_ENERGY = 4.0, 1.0


def factor(tau):
    """the per-hop forgetting factor of a time constant in seconds"""
    return float(np.exp(-0.016 / tau))


def hop_sum(q):
    """sum of the hop's 256 values in the contract's order: p[l] = ((q[l] + q[64 + l]) + q[128 + l]) + q[192 + l], then
    p[l] += p[l + off] for off = 32, 16 .. 1"""
    v = q.reshape(4, 64)
    p = ((v[0] + v[1]) + v[2]) + v[3]
    for off in (32, 16, 8, 4, 2, 1):
        p = p[:off] + p[off:2 * off]
    return float(p[0])


class DrcRef:
    """One stream.  run(x) takes whole hops, any number per call, and returns what those hops emit; the state is the contract's.
    a_hook: a function a [416] -> a [416] applied to the magnitudes of every emitted hop (the sensitivity experiment)."""

    def __init__(self, params=None, tau_peak=TAU_PEAK, tau_energy=TAU_ENERGY, equalise=True, ref_level=None, a_hook=None):
        self.p = params or S.Params()
        self.rho, self.lam = factor(tau_peak), factor(tau_energy)
        self.equalise, self.ref_level, self.a_hook = bool(equalise), ref_level, a_hook
        m = np.arange(1, 64, 2)
        self.taps = 2.0 / (np.pi * m) * (0.54 + 0.46 * np.cos(np.pi * m / 64.0))        # h[2 k + 1]; h[-m] = -h[m]
        self.reset()

    def reset(self):
        self.hist = np.zeros(HIST, dtype=np.float32)
        self.eh = self.M = self.Ein = self.Eout = self.g_prev = 0.0
        self.count = 0

    def state(self):
        return {'hist': self.hist.copy(), 'eh': self.eh, 'M': self.M, 'Ein': self.Ein, 'Eout': self.Eout, 'g_prev': self.g_prev,
                'count': self.count}

    def _emit(self, x):
        """the hop before ``x`` from hist and the first 144 samples of x -> (out float32 [256], y, gain, e0, e-hat)"""
        p = self.p
        win = np.concatenate([self.hist, x[:LOOK]]).astype(np.float64)          # s[256 j - 144 .. 256 j + 400)
        # 1. a[i], i = 256 j - 80 + q: win index 64 + q
        c = 64 + np.arange(416)
        sh = np.zeros(416)
        for k in range(32):
            sh = sh + self.taps[k] * (win[c - (2 * k + 1)] - win[c + (2 * k + 1)])
        a = np.sqrt(win[c] * win[c] + sh * sh)
        if self.count == 1:
            a[:80] = 0.0                                                        # before the stream's start
        if self.a_hook is not None:
            a = self.a_hook(a)
        # 2. the centred mean, in index order
        acc = np.zeros(HOP)
        for k in range(161):
            acc = acc + a[k:k + HOP]
        e = acc / 161.0
        # 3. attack / release
        eh = np.empty(HOP)
        prev = self.eh
        for n in range(HOP):
            cc = p.attack if e[n] >= prev else p.release
            prev = cc * prev + (1.0 - cc) * e[n]
            eh[n] = prev
        self.eh = prev
        # 4. the reference level
        self.M = max(float(e.max()), self.rho * self.M)
        e0 = p.e0_ratio * self.M if self.ref_level is None else float(self.ref_level)
        # 5. the curve
        s = win[LOOK:LOOK + HOP]
        g1 = np.ones(HOP)
        if e0 > 0:
            xin = 20.0 * np.log10(np.maximum(eh, 1e-10 * e0) / e0)
            g1 = 10.0 ** ((S.curve(xin, p.knots) - xin) / 20.0)
        y = g1 * s
        # 6. the equaliser
        g = 1.0
        if self.equalise:
            self.Ein = self.lam * self.Ein + hop_sum(s * s)
            self.Eout = self.lam * self.Eout + hop_sum(y * y)
            g = float(np.sqrt(self.Ein / self.Eout)) if self.Eout > 0 else 1.0
        gp = 1.0 if self.count == 1 else self.g_prev
        r = gp + (g - gp) * np.arange(1, HOP + 1) / 256.0
        self.g_prev = g
        return (y * r).astype(np.float32), y * r, g1 * r, e0, eh

    def run(self, x):
        """x float32 [nh * 256] -> dict: out float32 [nh * 256], out64 (before the float32 rounding), gain [nh * 256], level [nh],
        ehat [nh * 256] (zeros in the stream's first hop)"""
        x = np.asarray(x)
        assert x.dtype == np.float32 and x.ndim == 1 and len(x) % HOP == 0 and len(x) > 0
        nh = len(x) // HOP
        r = {'out': np.zeros(nh * HOP, np.float32), 'out64': np.zeros(nh * HOP), 'gain': np.zeros(nh * HOP), 'level': np.zeros(nh),
             'ehat': np.zeros(nh * HOP)}
        for h in range(nh):
            xh, cols = x[h * HOP:(h + 1) * HOP], slice(h * HOP, (h + 1) * HOP)
            if self.count >= 1:
                r['out'][cols], r['out64'][cols], r['gain'][cols], r['level'][h], r['ehat'][cols] = self._emit(xh)
            self.count = min(self.count + 1, 2)
            self.hist = np.concatenate([self.hist, xh])[-HIST:]                 # 7.
        return r


def compress_stream(x, **kw):
    """a whole signal (float32, any length) through a fresh DrcRef: zero-padded to whole hops, one zero hop behind it to flush the last
    one, the output realigned and cut -> float32 [len(x)]"""
    x = np.asarray(x, dtype=np.float32)
    nh = -(-len(x) // HOP)
    d = np.zeros((nh + 1) * HOP, np.float32)
    d[:len(x)] = x
    return DrcRef(**kw).run(d)['out'][HOP:HOP + len(x)]
