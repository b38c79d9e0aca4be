"""The shoebox image-source impulse response of DESIGN.md section 13 in numpy float64: the reference nele_rir_synth is tested against.

A room is 15 numbers: sizes L [3], source s [3], receiver m [3] (metres, both strictly inside) and beta[a][0], beta[a][1] in [0, 1]
(reflection factor of the wall at coordinate 0 / at L_a of axis a).  For axis a, parity u in {0, 1} and integer l
    delta_a(u, l) = (1 - 2u) s_a + 2 l L_a - m_a,     g_a(u, l) = beta[a][0]^|l - u| beta[a][1]^|l|     (0^0 = 1);
an image is a triple of (u, l): d = sqrt(sum delta_a^2), A = g_x g_y g_z / (4 pi d), tau = d fs / c, and for 0 <= n < taps
    h[n] = sum over the images with |n - tau| <= W of A sinc(n - tau) 0.5 (1 + cos(pi (n - tau) / W)).
Every image with tau - W <= taps - 1 is summed: the whole lattice box that can hold one is enumerated, no reflection-order cap."""
import numpy as np


def axis_images(L, s, m, beta0, beta1, dmax):
    """every (u, l) of one axis with |delta| <= dmax -> (delta, g) arrays"""
    deltas, gains = [], []
    lmax = int(np.ceil((dmax + abs(s) + abs(m)) / (2.0 * L))) + 1
    l = np.arange(-lmax, lmax + 1)
    for u in (0, 1):
        delta = (1 - 2 * u) * s + 2.0 * l * L - m
        with np.errstate(all='ignore'):
            g = np.power(float(beta0), np.abs(l - u).astype(np.float64)) * np.power(float(beta1), np.abs(l).astype(np.float64))
        keep = np.abs(delta) <= dmax
        deltas.append(delta[keep])
        gains.append(g[keep])
    return np.concatenate(deltas), np.concatenate(gains)


def images(room, taps, fs=16000.0, c=343.0, W=40):
    """-> (tau, A) of every image with tau - W <= taps - 1 (float64 arrays)"""
    room = np.asarray(room, dtype=np.float64).reshape(-1)
    L, s, m, beta = room[0:3], room[3:6], room[6:9], room[9:15].reshape(3, 2)
    dmax = (taps - 1 + W) * c / fs * (1.0 + 1e-9)
    ax = [axis_images(L[a], s[a], m[a], beta[a, 0], beta[a, 1], dmax) for a in range(3)]
    taus, amps = [], []
    for dx, gx in zip(*ax[0]):                                # one x image at a time keeps the arrays small
        d2 = dx * dx + ax[1][0][:, None] ** 2 + ax[2][0][None, :] ** 2
        d = np.sqrt(d2)
        tau = d * fs / c
        keep = tau - W <= taps - 1
        g = gx * ax[1][1][:, None] * ax[2][1][None, :]
        taus.append(tau[keep])
        amps.append((g / (4.0 * np.pi * d))[keep])
    return np.concatenate(taus), np.concatenate(amps)


def rir(room, taps, fs=16000.0, c=343.0, W=40):
    """-> (h [taps], SA [taps]): the response and, per tap, the sum of |A| over the images that reach it"""
    tau, A = images(room, taps, fs, c, W)
    first = np.ceil(tau - W).astype(np.int64)                 # first tap with n - tau >= -W
    h, SA = np.zeros(taps), np.zeros(taps)
    for j in range(2 * W + 1):
        n = first + j
        x = n - tau
        ok = (n >= 0) & (n < taps) & (np.abs(x) <= W)
        xo = x[ok]
        term = A[ok] * np.sinc(xo) * 0.5 * (1.0 + np.cos(np.pi * xo / W))
        h += np.bincount(n[ok], weights=term, minlength=taps)[:taps]
        SA += np.bincount(n[ok], weights=np.abs(A[ok]), minlength=taps)[:taps]
    return h, SA


def t60(h, fs=16000.0):
    """three times the span between the -5 dB and -25 dB crossings of the Schroeder energy decay curve (linear interpolation between the
    last sample above a level and the first at or below it), seconds"""
    h = np.asarray(h, dtype=np.float64)
    e = np.cumsum((h * h)[::-1])[::-1]
    with np.errstate(divide='ignore'):
        db = 10.0 * np.log10(e / e[0])

    def crossing(level):
        i = int(np.argmax(db <= level)) if (db <= level).any() else len(db)
        hi = db[i - 1]
        lo = db[i] if i < len(db) else -np.inf
        return (i - 1) + (0.0 if np.isinf(lo) else (hi - level) / (hi - lo))
    return 3.0 * (crossing(-25.0) - crossing(-5.0)) / fs
