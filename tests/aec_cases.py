"""The echo-cancellation scenario shared by tests/test_aec_cpu.py and tests/test_aec_gpu.py: the toy corpus as far-end speech and
near-end noise, a synthetic exponentially decaying echo path, the microphone = echo + noise at a stated echo-to-noise ratio."""
import os

import numpy as np

HERE = os.path.dirname(__file__)
TOY = os.path.join(HERE, 'golden', 'toy')
HOP = 256
_AUDIO = {}


def far_and_near():
    """far end: toy Train_Clean followed by toy Test_Clean (264 hops); near end: the two toy noise files over the same spans"""
    if not _AUDIO:
        from nele_gan_amd import dataio
        c0, _ = dataio.load(os.path.join(TOY, 'Train_Clean.wav'))
        n0, _ = dataio.load(os.path.join(TOY, 'Train_Noise.wav'))
        c1, _ = dataio.load(os.path.join(TOY, 'Test_Clean.wav'))
        n1, _ = dataio.load(os.path.join(TOY, 'Test_Noise.wav'))
        _AUDIO['far'] = np.concatenate([c0, c1]).astype(np.float64)
        _AUDIO['near'] = np.concatenate([n0[:len(c0)], n1[:len(c1)]]).astype(np.float64)
        assert len(_AUDIO['far']) == len(_AUDIO['near']) == 264 * HOP
    return _AUDIO['far'], _AUDIO['near']


def echo_path(seed, taps, t60):
    """h[n] = g[n] 10^(-3 n / (16000 T60)), g standard normal; 40 samples of bulk delay, a unit direct path; sum h^2 = 0.25"""
    g = np.random.default_rng(seed).standard_normal(taps)
    h = g * 10.0 ** (-3.0 * np.arange(taps) / (16000.0 * t60))
    h[:40] = 0.0
    h[40] = 1.0
    return h * np.sqrt(0.25 / np.sum(h * h))


def scale_to_enr(echo, noise, enr_db):
    return noise * np.sqrt(np.sum(echo * echo) / (np.sum(noise * noise) * 10.0 ** (enr_db / 10.0)))


def scenario(seed, taps, t60, enr_db, shift=0, hops=264):
    """-> dict: played (float32, the far end), h, echo, noise (float64) and mic = float32(echo + noise), ``hops`` hops each.  Streams
    of one batch differ in seed (the path) and shift (a circular shift of the far end, twice that of the near end)."""
    far, near = far_and_near()
    n = hops * HOP
    played = np.roll(far, shift)[:n].astype(np.float32)
    h = echo_path(seed, taps, t60)
    echo = np.convolve(played.astype(np.float64), h)[:n]
    noise = scale_to_enr(echo, np.roll(near, 2 * shift)[:n], enr_db) if enr_db is not None else np.zeros(n)
    return {'played': played, 'h': h, 'echo': echo, 'noise': noise, 'mic': (echo + noise).astype(np.float32)}


def reduction_db(echo, y):
    """second-half echo reduction, 10 log10(sum echo^2 / sum (echo - y)^2)"""
    half = len(echo) // 2
    return 10.0 * np.log10(np.sum(echo[half:] ** 2) / np.sum((echo[half:] - y[half:]) ** 2))
