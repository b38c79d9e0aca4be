"""numpy float64 restatement of the SSDRC specification of DESIGN.md section 11 (test infrastructure, like tests/p56_ref.py): one row at a
time, frame by frame, with numpy's FFT - nothing of the HIP kernels' structure (frame pairs, tiles, blocks)."""
import dataclasses

import numpy as np

N, HOP = 512, 256


@dataclasses.dataclass
class Params:
    shape: bool = True
    compress: bool = True
    lifter_q: int = 20
    beta: float = 0.25
    preemph: float = 0.3
    attack: float = 1e-4
    release: float = 0.15
    e0_ratio: float = 0.3
    knots: tuple = ((-100.0, -100.0), (-60.0, -45.0), (-30.0, -15.0), (0.0, 0.0))


def window():
    n = np.arange(N)
    return np.sqrt(0.5 - 0.5 * np.cos(2.0 * np.pi * n / N))


def fixed_shaping():
    k = np.arange(N)
    f = 31.25 * np.minimum(k, N - k)
    db = np.where(f < 500.0, -6.0 * np.log2(500.0 / np.maximum(f, 31.25)),
                  np.where(f <= 1000.0, 0.0, np.where(f <= 4000.0, 12.0 * np.log2(np.maximum(f, 1.0) / 1000.0), 24.0)))
    return 10.0 ** (db / 20.0), np.maximum(f - 1000.0, 0.0) / 7000.0


def frames_of(x):
    """-> [T, 512]: frame t covers [256 t - 256, 256 t + 256), t = 0 .. ceil(L / 256), zeros outside [0, L)"""
    L = len(x)
    T = -(-L // HOP) + 1
    pad = np.zeros(HOP * (T + 1))
    pad[HOP:HOP + L] = x
    return np.stack([pad[HOP * t:HOP * t + N] for t in range(T)])


def voicing(fr):
    rms = np.sqrt(np.mean(fr ** 2, axis=1))
    z = np.sum(fr[:, 1:] * fr[:, :-1] < 0, axis=1)
    v = rms / np.maximum(z, 1)
    m = v.max()
    return v / m if m > 0 else np.zeros_like(v)


def shape(x, p=None, gains=None):
    """stage 1 of one row (float64 in and out).  ``gains``: 'unity' replaces every spectral gain by 1 (the analysis / synthesis identity)."""
    p = p or Params()
    x = np.asarray(x, dtype=np.float64)
    L = len(x)
    fr = frames_of(x)
    T = fr.shape[0]
    w = window()
    hr, pre = fixed_shaping()
    pv = voicing(fr)
    lifter = np.zeros(N)
    lifter[2:p.lifter_q + 1] = 1.0
    lifter[N - p.lifter_q:N - 1] = 1.0
    out = np.zeros(HOP * (T + 1))
    for t in range(T):
        X = np.fft.fft(w * fr[t])
        if gains == 'unity':
            Y = X
        else:
            l_ = 0.5 * np.log(np.maximum(np.abs(X) ** 2, 1e-20))
            c = np.real(np.fft.ifft(l_))
            ln_et = np.real(np.fft.fft(c * lifter))
            Y = X * np.exp(p.beta * pv[t] * ln_et) * (1.0 + p.preemph * pv[t] * pre) * hr
        out[HOP * t:HOP * t + N] += w * np.real(np.fft.ifft(Y))
    return out[HOP:HOP + L]


def hilbert_fir():
    m = np.arange(-64, 65)
    h = np.zeros(129)
    odd = (m % 2) != 0
    h[odd] = 2.0 / (np.pi * m[odd])
    return h * (0.54 + 0.46 * np.cos(np.pi * m / 64.0))


def envelope(s):
    L = len(s)
    sh = np.convolve(s, hilbert_fir())[64:64 + L]
    a = np.sqrt(s ** 2 + sh ** 2)
    return np.convolve(a, np.ones(161))[80:80 + L] / 161.0


def smooth(e, attack, release):
    eh = np.empty_like(e)
    prev = 0.0
    for n in range(len(e)):
        a = attack if e[n] >= prev else release
        prev = a * prev + (1.0 - a) * e[n]
        eh[n] = prev
    return eh


def curve(xin, knots):
    kx = np.asarray([k[0] for k in knots], dtype=np.float64)
    ky = np.asarray([k[1] for k in knots], dtype=np.float64)
    out = np.interp(xin, kx, ky)                            # constant above the last knot
    return np.where(xin < kx[0], xin + (ky[0] - kx[0]), out)


def compress(s, p=None):
    """stage 2 of one row -> (y before the energy scaling, e-hat)"""
    p = p or Params()
    s = np.asarray(s, dtype=np.float64)
    if len(s) == 0:
        return s.copy(), s.copy()
    e = envelope(s)
    eh = smooth(e, p.attack, p.release)
    e0 = p.e0_ratio * e.max()
    if e0 <= 0:
        return s.copy(), eh
    xin = 20.0 * np.log10(np.maximum(eh, 1e-10 * e0) / e0)
    return 10.0 ** ((curve(xin, p.knots) - xin) / 20.0) * s, eh


def ssdrc(x, p=None):
    """the full chain of one row: float32 / float64 samples in -> float64 out, scaled to the input's energy"""
    p = p or Params()
    x = np.asarray(x, dtype=np.float64)
    y = shape(x, p) if p.shape else x.copy()
    if p.compress:
        y = compress(y, p)[0]
    sx, sy = np.sum(x ** 2), np.sum(y ** 2)
    return y * np.sqrt(sx / sy) if sy > 0 else np.zeros_like(y)


# ------------------------------------------------------------------------------------------------ what the tests measure
def band_share(x, lo=1000.0, hi=4000.0, fs=16000.0):
    """share of the signal's energy between lo and hi Hz"""
    X = np.abs(np.fft.rfft(np.asarray(x, dtype=np.float64))) ** 2
    f = np.fft.rfftfreq(len(x), 1.0 / fs)
    return float(X[(f >= lo) & (f < hi)].sum() / X.sum())


def crest(x):
    x = np.asarray(x, dtype=np.float64)
    return float(np.abs(x).max() / np.sqrt(np.mean(x ** 2)))


def make_signal(L, seed):
    """two sinusoids and noise with a silent stretch (zero-crossing count 0, frames on the log floor), float32"""
    rng = np.random.RandomState(seed)
    n = np.arange(L)
    x = 0.3 * np.sin(2 * np.pi * 220.0 * n / 16000.0) + 0.1 * np.sin(2 * np.pi * 2500.0 * n / 16000.0 + 1.0) + 0.02 * rng.randn(L)
    x *= 0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * n / 16000.0)
    a, b_ = L // 5, L // 5 + max(3 * L // 5, 8)
    x[a:b_] = 0.0
    return x.astype(np.float32)
