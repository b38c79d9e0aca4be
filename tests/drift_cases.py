"""The clock-drift scenario shared by tests/test_drift_cpu.py and tests/test_drift_gpu.py: tests/aec_cases.py's audio tiled to the run's
length, its synthetic echo path behind a bulk delay, and a microphone whose clock runs fast by `ppm` parts per million - its echo is the
loudspeaker's echo read at n (1 + ppm 1e-6) - bulk through a 48-tap Kaiser (beta 9) windowed sinc, which is NOT the compensator's table."""
import numpy as np

import aec_cases as C

HOP = C.HOP
RES_TAPS, RES_BETA = 48, 9.0


def tiled(sig, n, shift=0):
    return np.roll(np.tile(sig, -(-n // len(sig))), shift)[:n]


def read_at(sig, pos):
    """sig at the fractional positions pos (zeros outside it): 48 taps of sinc(m - frac) under a Kaiser window over |m - frac| <= 24"""
    i0 = np.floor(pos).astype(np.int64)
    frac = pos - i0
    half = RES_TAPS // 2
    out = np.zeros(len(pos))
    for m in range(-half + 1, half + 1):
        t = m - frac
        w = np.sinc(t) * np.i0(RES_BETA * np.sqrt(np.maximum(0.0, 1.0 - (t / half) ** 2))) / np.i0(RES_BETA)
        idx = i0 + m
        ok = (idx >= 0) & (idx < len(sig))
        out += np.where(ok, w * sig[np.clip(idx, 0, len(sig) - 1)], 0.0)
    return out


def scenario(ppm, enr_db, seed, hops, bulk=2000, taps=700, t60=0.08, shift=0, silent=False):
    """-> dict: played (float32), h, echo (float64: what of `played` the drifting microphone hears), noise (float64) and mic =
    float32(echo + noise).  enr_db None: no near-end noise; silent: `played` is zeros.  Streams of one batch differ in seed and shift as
    in aec_cases.scenario."""
    far, near = C.far_and_near()
    n = hops * HOP
    played = (np.zeros(n) if silent else tiled(far, n, shift)).astype(np.float32)
    h = C.echo_path(seed, taps, t60)
    at_speaker = np.convolve(played.astype(np.float64), h)[:n]
    echo = read_at(at_speaker, np.arange(n) * (1.0 + ppm * 1e-6) - bulk)
    noise = tiled(near, n, 2 * shift)
    if enr_db is not None and not silent:
        noise = C.scale_to_enr(echo, noise, enr_db)
    elif enr_db is None:
        noise = np.zeros(n)
    return {'played': played, 'h': h, 'echo': echo, 'noise': noise, 'mic': (echo + noise).astype(np.float32)}


def echo_free(hops, shift=0):
    """a microphone that hears the toy noise only, against the speech far end"""
    far, near = C.far_and_near()
    n = hops * HOP
    return {'played': tiled(far, n, shift).astype(np.float32), 'mic': tiled(near, n, 2 * shift).astype(np.float32)}


# tests/test_drift_gpu.py's closed-loop scenarios: blocks -> per slot (base in hops, bulk in samples); 264 hops at +500 ppm, ENR 10 dB,
# seeds and shifts per stream as tests/test_aec_gpu.py's
GPU_HOPS, GPU_PPM, GPU_ENR = 264, 500.0, 10.0
GPU_LOOPS = {4: [(2, 600), (2, 600), (2, 600)], 7: [(5, 1400), (5, 1400)]}
# the reference's own sensitivity on those scenarios (tests/test_drift_cpu.py measures it: 3.95e-9 samples), rounded up: how far tau
# ends from an unperturbed run when tau and C_s are moved by 1e-15 relative after every hop
PERTURBED_TAU = 4e-9
PERTURBED_RATE = 1.5e-13                                    # the same for rate (measured: 1.4e-13)
_GPU = {}


def gpu_loop(blocks, slot):
    if (blocks, slot) not in _GPU:
        _GPU[(blocks, slot)] = scenario(GPU_PPM, GPU_ENR, 11 + slot, GPU_HOPS, bulk=GPU_LOOPS[blocks][slot][1], shift=4001 * slot)
    return _GPU[(blocks, slot)]


def window_db(echo, y, a, b):
    """echo reduction over hops a .. b - 1"""
    sl = slice(a * HOP, b * HOP)
    return 10.0 * np.log10(np.sum(echo[sl] ** 2) / np.sum((echo[sl] - y[sl]) ** 2))
