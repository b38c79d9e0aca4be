"""The residual-echo suppression scenarios shared by tests/test_res_cpu.py and tests/test_res_gpu.py: tests/aec_cases.py's scenario
through the reference canceller, its float32 residual and echo through the reference suppressor, and the two figures of DESIGN.md
section 17 - how much of the residual echo the gains take out and what they do to the noise."""
import numpy as np

import aec_cases as C
from aec_ref import AecRef
from res_ref import HOP, ResRef, apply_gains

# (seed, taps, T60, ENR dB, partitions): the three scenarios of DESIGN.md section 17's table
SCENARIOS = ((1, 700, 0.08, 10.0, 3), (1, 1800, 0.25, 10.0, 8), (2, 700, 0.08, 20.0, 3))
_RUNS = {}


def ref_run(seed, taps, t60, enr_db, P):
    """the scenario through AecRef(P) and ResRef(): computed once, shared, never changed
    -> dict: e, y (float32: what the kernel would be given), out (float32), G [264, 257], noise (float64)"""
    key = (seed, taps, t60, enr_db, P)
    if key not in _RUNS:
        s = C.scenario(seed, taps, t60, enr_db)
        e, y = AecRef(P).run(s['mic'], s['played'])
        e, y = e.astype(np.float32), y.astype(np.float32)
        out, G = ResRef().run(e, y)
        _RUNS[key] = {'e': e, 'y': y, 'out': out, 'G': G, 'noise': s['noise']}
    return _RUNS[key]


def figures(e, noise, out, G):
    """-> (suppression of the residual echo in dB, change of the noise level in dB, largest |echo part + noise part - out| / max |out|)
    over the second half of the hops.  The residual echo is e - noise; the parts are apply_gains of it and of the noise; the unprocessed
    signals are read one hop earlier than the output, which is one hop late."""
    nh = len(G)
    half, late = slice(nh // 2 * HOP, nh * HOP), slice((nh // 2 - 1) * HOP, (nh - 1) * HOP)
    r = e.astype(np.float64) - noise
    pe, pn = apply_gains(G, r).astype(np.float64), apply_gains(G, noise).astype(np.float64)
    sup = 10.0 * np.log10(np.sum(r[late] ** 2) / np.sum(pe[half] ** 2))
    lvl = 10.0 * np.log10(np.sum(pn[half] ** 2) / np.sum(noise[late] ** 2))
    split = float(np.abs(pe + pn - out.astype(np.float64)).max() / np.abs(out).max())
    return float(sup), float(lvl), split
