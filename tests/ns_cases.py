"""The noise-suppression scenarios and every bound shared by tests/test_ns_cpu.py and tests/test_ns_gpu.py: the toy far end of
tests/aec_cases.py as the near-end talker, stationary synthetic noise (white, or pink through a fixed third-order filter) scaled to a
stated SNR over the whole signal, the figures of DESIGN.md section 21, and the sensitivity experiment the GPU bounds stand on.  Each
bound has the value measured with tests/ns_ref.py beside it."""
import numpy as np
from scipy.signal import lfilter

import aec_cases as C
from ns_ref import HOP, NsRef, apply_gains

PINK_B = [0.049922035, -0.095993537, 0.050612699, -0.004408786]
PINK_A = [1, -2.494956002, 2.017265875, -0.522189400]
# (noise, SNR dB): the three rows of DESIGN.md section 21's table
SCENARIOS = (('pink', 0.0), ('pink', 10.0), ('white', 0.0))

# ---- bounds of the figures (second half of the 264 hops)        measured with ns_ref:   pink 0 dB   pink 10 dB   white 0 dB
MIN_NOISE_ATTENUATION_DB = 6.0                                  # noise attenuated, dB:     10.21       7.56         8.77
MIN_SPEECH_LEVEL_CHANGE_DB = -1.5                               # speech level change, dB:  -1.26       -0.23        -0.59
MAX_ERROR_RATIO_OF_INPUTS = 0.5                                 # error after / before:     0.166       0.261        0.170
#                                                                 (sum (out - speech)^2 / sum speech^2: 1.018 -> 0.169, 0.102 -> 0.027,
#                                                                  0.998 -> 0.169)
MAX_SPLIT = 3 * 2.0 ** -24                                      # |speech part + noise part - out| / peak: 8.9e-8, 7.7e-8, 7.4e-8
# ---- the noise step: pink noise alone (rms 0.01), +10 dB at hop 300, 700 hops; the level is the mean periodogram behind the step
STEP_HOP, STEP_DB, STEP_HOPS_TOTAL = 300, 10.0, 700
STEP_MAX_HOPS, STEP_WITHIN_DB = 360, 3.0                        # three minima windows; measured: within 3 dB 274 hops after the step,
#                                                                 the last 40 hops 0.55 dB above the level (the beta = 1.47 bias)
# ---- sensitivity: every Y2f one float32 ulp up or down at random, three seeds, the largest deviation over the seeds, measured with
# ns_ref on the inputs of the GPU parity shapes and rounded up to two digits (tests/test_ns_cpu.py measures them again); no I or q
# decision changed in any of them.  gains, presence: absolute; noise_psd: relative; out: over the output's peak.
SENS = {
    ('pink', 10.0, 40): {'gains': 3.1e-7, 'presence': 5.3e-7, 'noise_psd': 4.6e-7, 'out': 6.2e-8},      # shape (1, 40)
    ('pink', 0.0, 264): {'gains': 5.3e-7, 'presence': 1.0e-6, 'noise_psd': 1.02e-6, 'out': 9.6e-8},     # shape (3, 264), stream 0
    ('pink', 10.0, 264): {'gains': 6.5e-7, 'presence': 5.3e-7, 'noise_psd': 4.6e-7, 'out': 8.0e-8},     # stream 1
    ('white', 0.0, 264): {'gains': 3.8e-7, 'presence': 5.6e-7, 'noise_psd': 4.3e-7, 'out': 8.8e-8},     # stream 2
}
SENS_INPUTS = tuple(k for k in SENS)
# The GPU bounds are 8 x these, per stream: a GPU run flips few roundings where the experiment flips all; the factor covers the spread
# between seeds and the exp / log / E1 implementations.  So, for instance, |G_gpu - G_ref| <= 2.5e-6 at shape (1, 40).
# Measured on an MI355X (largest over both shapes and every stream): gains 1.8e-15, presence 2.3e-16, noise_psd 6.7e-16 relative,
# out 1.1e-17 of the peak - the kernel's Y2f rounds as numpy's does on these inputs, so no rounding flipped.
GPU_FACTOR = 8.0
GPU_FIGURES_WITHIN_DB = 0.02
_CACHE = {}


def noise(kind, n):
    v = np.random.default_rng(7).standard_normal(n)
    return v if kind == 'white' else lfilter(PINK_B, PINK_A, v)


def scenario(kind, snr_db, hops=264):
    """-> dict: speech, noise (float64) and x = float32(speech + noise), ``hops`` hops each; the noise is scaled to the SNR over the
    whole 264-hop signal and then cut"""
    key = ('s', kind, snr_db, hops)
    if key not in _CACHE:
        speech, _ = C.far_and_near()
        v = noise(kind, len(speech))
        v = v * np.sqrt(np.sum(speech * speech) / (np.sum(v * v) * 10.0 ** (snr_db / 10.0)))
        n = hops * HOP
        _CACHE[key] = {'speech': speech[:n], 'noise': v[:n], 'x': (speech[:n] + v[:n]).astype(np.float32)}
    return _CACHE[key]


def ref_run(kind, snr_db, hops=264):
    """the scenario through NsRef(): computed once, shared, never changed"""
    key = ('r', kind, snr_db, hops)
    if key not in _CACHE:
        _CACHE[key] = NsRef().run(scenario(kind, snr_db, hops)['x'])
    return _CACHE[key]


def figures(speech, noise, out, G):
    """-> (noise attenuated dB, speech level change dB, error ratio before, after, largest |speech part + noise part - out| / max |out|)
    over the second half of the hops.  The parts are apply_gains of the speech and of the noise (the float32 rounding of the input is
    left with the noise); the unprocessed signals are read one hop earlier than the output, which is one hop late."""
    nh = len(G)
    half, late = slice(nh // 2 * HOP, nh * HOP), slice((nh // 2 - 1) * HOP, (nh - 1) * HOP)
    ps, pn = apply_gains(G, speech).astype(np.float64), apply_gains(G, noise).astype(np.float64)
    att = 10.0 * np.log10(np.sum(noise[late] ** 2) / np.sum(pn[half] ** 2))
    lvl = 10.0 * np.log10(np.sum(ps[half] ** 2) / np.sum(speech[late] ** 2))
    s2 = np.sum(speech[late] ** 2)
    before = np.sum(noise[late] ** 2) / s2
    after = np.sum((out.astype(np.float64)[half] - speech[late]) ** 2) / s2
    split = float(np.abs(ps + pn - out.astype(np.float64)).max() / np.abs(out).max())
    return float(att), float(lvl), float(before), float(after), split


def flip_hook(seed):
    """Y2f -> Y2f with every element one float32 ulp up or down at random"""
    rng = np.random.default_rng(seed)

    def hook(y2):
        up = rng.integers(0, 2, y2.shape).astype(bool)
        return np.where(up, np.nextafter(y2, np.float32(np.inf)), np.nextafter(y2, np.float32(0))).astype(np.float32)
    return hook


def sensitivity(x, base, seeds=(1, 2, 3)):
    """the all-flipped experiment on input x against the unperturbed run ``base`` -> dict of the largest deviations over the seeds:
    gains, presence (absolute), noise_psd (relative), out (over the peak of base's output), and decisions (how many I or q == 0 / 1
    decisions changed)"""
    worst = {'gains': 0.0, 'presence': 0.0, 'noise_psd': 0.0, 'out': 0.0, 'decisions': 0}
    peak = float(np.abs(base['out']).max())
    for seed in seeds:
        r = NsRef(y2_hook=flip_hook(seed)).run(x)
        worst['gains'] = max(worst['gains'], float(np.abs(r['gains'] - base['gains']).max()))
        worst['presence'] = max(worst['presence'], float(np.abs(r['presence'] - base['presence']).max()))
        worst['noise_psd'] = max(worst['noise_psd'], float(np.abs(r['noise_psd'] / base['noise_psd'] - 1.0).max()))
        worst['out'] = max(worst['out'], float(np.abs(r['out'].astype(np.float64) - base['out']).max()) / peak)
        fr = ~np.isnan(base['I'][:, 0])
        worst['decisions'] += int(np.sum(r['I'][fr] != base['I'][fr]) + np.sum((r['q'][fr] == 1) != (base['q'][fr] == 1))
                                  + np.sum((r['q'][fr] == 0) != (base['q'][fr] == 0)))
    return worst
