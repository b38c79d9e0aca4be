"""Inputs of the running-ESTOI tests (tests/test_monitor_cpu.py for the premises and the tie to oracle/estoi.py,
tests/test_monitor_gpu.py on the device).  Plain module: numpy, tests/estoi_cases.py and tests/monitor_ref.py; nothing here touches a
GPU.  A case is a pair (ref, deg) of float32 signals at 16 kHz, a whole number of 256-sample hops:
  steady        estoi_cases.noise_pair(256 * 40, 11): every frame is kept; 40 hops cross the 31 kept frames of the first segment
  gapped        311 frames of which 278 are kept, in four runs; gapped_boost: its first 0.1 s six times louder - 256 kept, the nearest
                frame 0.088 dB from the gate
  quiet_start   0.5 s at -50 dB, then steady noise: the running maximum keeps the quiet frames that the global one drops
  long_gap      two kept runs with 40 dropped frames between them: the ring spans the gap
  silence       digital silence: every frame is kept, every segment skipped
  nan_deg       steady noise whose deg is not a number for hop 20: the segments that hold it are skipped, 30 kept frames long
  nan_both      the same with ref not a number too: the frames are dropped and never reach the ring"""
import functools

import numpy as np

import estoi_cases as EC
import monitor_ref as R

HOP = R.HOP
NAMES = ('steady', 'gapped', 'gapped_boost', 'quiet_start', 'long_gap', 'silence', 'nan_deg', 'nan_both')
ORACLE_NAMES = ('steady', 'gapped', 'gapped_boost')          # the causal gate equals the global one on every frame
# name -> (hops, frames seen, frames kept)
EXPECTED = {
    'steady': (40, 48, 48),
    'gapped': (250, 311, 278),
    'gapped_boost': (250, 311, 256),
}


def _gapped(boost):
    L = 64000
    t = np.arange(L) / 16000.0
    rng = np.random.default_rng(5)
    env = 0.02 * (1.2 + np.sin(2 * np.pi * 3.1 * t)) * (1 + 0.5 * np.sin(2 * np.pi * 0.7 * t + 1))
    x = env * rng.standard_normal(L)
    for a, b in EC.GAPS:
        x[a:b] *= 1e-4
    if boost:
        x[:1600] *= 6
    y = x + 0.03 * rng.standard_normal(L)
    return x.astype(np.float32), y.astype(np.float32)


def _noise(L, seed, scale=None):
    """estoi_cases.noise_pair's signals, the clean one scaled by scale [L] before the degraded one is formed"""
    rng = np.random.default_rng(seed)
    x = 0.03 * rng.standard_normal(L)
    if scale is not None:
        x = x * scale
    y = x + 0.03 * rng.standard_normal(L)
    return x.astype(np.float32), y.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == 'steady':
        x, y = EC.noise_pair(HOP * 40, 11)
    elif name in ('gapped', 'gapped_boost'):
        x, y = _gapped(name == 'gapped_boost')
    elif name == 'quiet_start':
        s = np.ones(HOP * 72)
        s[:8000] = 10.0 ** (-50 / 20.0)
        x, y = _noise(HOP * 72, 12, s)
    elif name == 'long_gap':
        s = np.ones(HOP * 124)
        s[HOP * 45:HOP * 79] = 1e-4                         # 8704 samples = 5440 at 10 kHz: 40 whole frames and more
        x, y = _noise(HOP * 124, 13, s)
    elif name == 'silence':
        x, y = np.zeros(HOP * 45, dtype=np.float32), np.zeros(HOP * 45, dtype=np.float32)
    elif name in ('nan_deg', 'nan_both'):
        x, y = (a.copy() for a in EC.noise_pair(HOP * 90, 14))
        y[HOP * 20:HOP * 21] = np.nan
        if name == 'nan_both':
            x[HOP * 20:HOP * 21] = np.nan
    else:
        raise KeyError(name)
    assert len(x) % HOP == 0 and x.dtype == np.float32 and y.dtype == np.float32
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


ALPHA = R.alpha_of(0.25)


@functools.lru_cache(maxsize=None)
def reference(name, lag=0):
    """the streaming reference on the whole case (computed once, shared, not to be written to)"""
    x, y = case(name)
    return R.run(x, y, lag=lag, alpha=ALPHA)


def margin(frames):
    """the smallest distance in dB of any frame with a finite energy from the causal gate"""
    d = [abs(m - 40.0 - en) for (en, m, _) in frames if np.isfinite(en)]
    return min(d) if d else np.inf
