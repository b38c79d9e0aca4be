"""The bulk-delay scenarios shared by tests/test_bulk_cpu.py and tests/test_bulk_gpu.py: tests/aec_cases.py's audio (the toy corpus
as far-end speech and near-end noise, 264 hops), an exponentially decaying echo path behind ``bulk`` samples of pure delay, the
microphone = echo + noise at a stated echo-to-noise ratio; and microphones without any echo, which must never lock."""
import numpy as np

import aec_cases as C

HOP = C.HOP
HOPS = 264


def path(seed, taps, t60, bulk):
    """h = [0 x bulk, g[n] 10^(-3 n / (16000 T60))], g standard normal with g[0] replaced by a unit direct path; sum h^2 = 0.25"""
    g = np.random.default_rng(seed).standard_normal(taps)
    h = g * 10.0 ** (-3.0 * np.arange(taps) / (16000.0 * t60))
    h[0] = 1.0
    h = np.concatenate([np.zeros(bulk), h])
    return h * np.sqrt(0.25 / np.sum(h * h))


def scenario(bulk, enr_db, seed, taps=700, t60=0.08, shift=0, hops=HOPS):
    """-> dict: played (float32, the far end), h, echo, noise (float64), mic = float32(echo + noise).  Streams of one batch differ in
    seed and shift (a circular shift of the far end, twice that of the near end)."""
    far, near = C.far_and_near()
    n = hops * HOP
    played = np.roll(far, shift)[:n].astype(np.float32)
    h = path(seed, taps, t60, bulk)
    echo = np.convolve(played.astype(np.float64), h)[:n]
    noise = C.scale_to_enr(echo, np.roll(near, 2 * shift)[:n], enr_db)
    return {'played': played, 'h': h, 'echo': echo, 'noise': noise, 'mic': (echo + noise).astype(np.float32), 'bulk': bulk}


def negatives():
    """-> [(name, mic, played)] float32, 264 hops each: microphones that hold no echo of `played`"""
    far, near = C.far_and_near()
    played = far.astype(np.float32)
    level = np.sqrt(np.mean(far * far))
    out = []
    for seed in range(8):
        out.append(('white noise, seed %d' % seed, (level * np.random.default_rng(seed).standard_normal(len(far))).astype(np.float32), played))
    for k in range(8):
        out.append(('toy noise shifted by %d' % (3001 * k), np.roll(near, 3001 * k).astype(np.float32), played))
    for k in range(8):
        out.append(('reversed far end shifted by %d' % (3001 * k), np.roll(far[::-1], 3001 * k).astype(np.float32), played))
    out.append(('played = 0', near.astype(np.float32), np.zeros_like(played)))
    return out
