"""numpy float64 restatement of the look-ahead true-peak limiter of DESIGN.md section 26 (test infrastructure, like tests/drc_ref.py):
one stream, hop by hop, with the contract's explicit state, written from the contract - nothing of the HIP kernel's structure (ring,
lanes, waves).  Sums are loops in index order (never np.sum: its pairwise order is not the contract's); max and min are np.fmax and
np.fmin, which pass over a NaN operand as section 26 (d) says, and a maximum starts from 0."""
import numpy as np

HOP, REACH, MAX_LOOKAHEAD = 256, 6, 192
HIST = HOP + REACH
CEILING = 10.0 ** (-1.0 / 20.0)
RELEASE = float(np.exp(-1.0 / (16000 * 0.1)))


def taps():
    """f[k - 1][m + 5] = sinc(m - k / 4) (0.5 + 0.5 cos(pi (m - k / 4) / 6)), k = 1 .. 3, m = -5 .. 6"""
    m = np.arange(-5, 7, dtype=np.float64)
    t = np.stack([m - k / 4.0 for k in (1, 2, 3)])
    return np.sinc(t) * (0.5 + 0.5 * np.cos(np.pi * t / 6.0))


def floor32(c):
    """the largest float32 <= c"""
    cf = np.float32(c)
    return cf if float(cf) <= c else np.nextafter(cf, np.float32(0))


def interpolated_max(s, f):
    """s [n + 11] -> [n]: max_k |u_k[i]| for the i whose s[i - 5] is s[0] .. , each u a sum over ascending m with unfused products"""
    n = len(s) - 11
    best = np.zeros(n)
    for k in range(3):
        u = np.zeros(n)
        for m in range(12):
            u = u + f[k, m] * s[m:m + n]
        best = np.fmax(best, np.abs(u))
    return best


def reduction(p, c):
    """step 2 (a NaN compares false: 1)"""
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(p > c, c / p, 1.0)


class LimRef:
    """One stream.  run(x) takes whole hops, any number per call, and returns what those hops emit; the state is the contract's:
    count, d, hist (the last 262 input samples, float32) and q (the last LA values)."""

    def __init__(self, ceiling=CEILING, drive=1.0, lookahead=80, rel=RELEASE, true_peak=True):
        assert ceiling > 0 and drive > 0 and 1 <= lookahead <= MAX_LOOKAHEAD and 0 <= rel < 1
        self.c, self.drive, self.LA, self.rel = float(ceiling), float(drive), int(lookahead), float(rel)
        self.f = taps() if true_peak else None
        self.cf = floor32(self.c)
        self.reset()

    def reset(self):
        self.hist = np.zeros(HIST, dtype=np.float32)
        self.q = np.zeros(self.LA)
        self.d = 0.0
        self.count = 0

    def state(self):
        return {'hist': self.hist.copy(), 'q': self.q.copy(), 'd': self.d, 'count': self.count}

    def _emit(self, x):
        """the hop before ``x`` from hist and the first LA + 6 samples of x -> (out float32 [256], y [256], gain [256], peak, r of the
        hop [256], the mean of q before it is held under r [256])"""
        LA, c = self.LA, self.c
        first = self.count == 1
        E = LA if first else 0                                           # the recursion starts LA samples before the stream
        # s[i], i = t0 - E - 6 .. t0 + 255 + LA + 6, t0 the emitted hop's first sample; hist is s[t0 - 6 .. t0 + 256) / drive
        s = self.drive * np.concatenate([np.zeros(E, np.float32), self.hist, x[:LA + REACH]]).astype(np.float64)
        n = E + HOP + LA                                                 # p[i], i = t0 - E .. t0 + 255 + LA, at [i - (t0 - E)]
        p = np.abs(s[REACH:REACH + n])
        if self.f is not None:
            um = interpolated_max(s, self.f)                             # u[i], i = t0 - E - 1 .. t0 + 255 + LA
            p = np.fmax(np.fmax(p, um[1:]), um[:-1])
        r = reduction(p, c)
        peak = float(np.fmax.reduce(np.concatenate([[0.0], p[E:E + HOP]])))
        m = r[:E + HOP].copy()                                           # 3.
        for k in range(1, LA + 1):
            m = np.fmin(m, r[k:k + E + HOP])
        q = np.empty(LA + HOP)                                           # q[n], n = t0 - LA .. t0 + 255
        q[:LA - E] = self.q[:LA - E] if not first else 0.0
        d = 0.0 if first else self.d
        for j in range(E + HOP):                                         # 4.
            d = max(1.0 - m[j], self.rel * d)
            q[LA - E + j] = 1.0 - d
        self.d = d
        self.q = q[HOP:].copy()
        acc = np.zeros(HOP)                                              # 5.
        for k in range(LA + 1):
            acc = acc + q[k:k + HOP]
        mean = acc / float(LA + 1)
        g = np.fmin(mean, r[E:E + HOP])                                  # held under r[n]: property (a) in every bit
        with np.errstate(over='ignore', invalid='ignore'):
            y = g * s[E + REACH:E + REACH + HOP]                         # 6.
            o = y.astype(np.float32)
        out = np.where(o > self.cf, self.cf, np.where(o < -self.cf, -self.cf, o)).astype(np.float32)
        return out, y, g, peak, r[E:E + HOP], mean

    def run(self, x):
        """x float32 [nh * 256] -> dict: out float32 [nh * 256], y (g s, float64, before the float32 rounding and the clamp), gain
        [nh * 256], peak [nh], r and mean (step 5's sum / (LA + 1), before the min) [nh * 256] (zeros in the stream's first hop)"""
        x = np.asarray(x)
        assert x.dtype == np.float32 and x.ndim == 1 and len(x) % HOP == 0 and len(x) > 0
        nh = len(x) // HOP
        res = {'out': np.zeros(nh * HOP, np.float32), 'y': np.zeros(nh * HOP), 'gain': np.zeros(nh * HOP), 'peak': np.zeros(nh),
               'r': np.zeros(nh * HOP), 'mean': np.zeros(nh * HOP)}
        for h in range(nh):
            xh, cols = x[h * HOP:(h + 1) * HOP], slice(h * HOP, (h + 1) * HOP)
            if self.count >= 1:
                res['out'][cols], res['y'][cols], res['gain'][cols], res['peak'][h], res['r'][cols], res['mean'][cols] = self._emit(xh)
            self.count = min(self.count + 1, 2)
            self.hist = np.concatenate([self.hist, xh])[-HIST:]
        return res


def limit_stream(x, **kw):
    """a whole signal (float32, any length) through a fresh LimRef: zero-padded to whole hops, one zero hop behind it to flush the last
    one, the outputs realigned and cut -> dict as LimRef.run's, each [len(x)] (peak: per hop)"""
    x = np.asarray(x, dtype=np.float32)
    nh = -(-len(x) // HOP)
    d = np.zeros((nh + 1) * HOP, np.float32)
    d[:len(x)] = x
    r = LimRef(**kw).run(d)
    return {k: (v[1:] if k == 'peak' else v[HOP:HOP + len(x)]) for k, v in r.items()}
