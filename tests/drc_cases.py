"""The scenarios and every bound shared by tests/test_drc_cpu.py and tests/test_drc_gpu.py: the toy far end of
tests/aec_cases.py as the speech, the four noises of tests/siiopt_cases.py, tests/siiopt_ref.py's chain as 'the rule's output', the
oracle's SIIB and ESTOI, and the sensitivity experiment the GPU bounds stand on.  Each bound has the value measured with
tests/drc_ref.py beside it."""
import numpy as np

import aec_cases as C
import siiopt_cases as SK
import ssdrc_ref as S
from drc_ref import HOP, DrcRef, compress_stream

# (noise, SNR dB, input): the five rows of DESIGN.md section 23's table; 'speech' is the plain speech, 'rule' the SII rule's output
ROWS = (('ssn', -5.0, 'speech'), ('ssn', -5.0, 'rule'), ('pink', -5.0, 'rule'), ('white', 0.0, 'rule'), ('lowpass', -5.0, 'rule'))

# ---- bounds of the figures (default parameters, the output read one hop late and scaled to the input's rms)
#                                         measured with drc_ref:  ssn speech  ssn rule  pink rule  white rule  low-pass rule
MIN_SIIB_RATIO = 1.15                   # raw SIIB out / in:        1.371       1.235     1.250      1.321       0.980 (no bound: see below)
SIIB_BOUND_ROWS = ROWS[:4]              # SIIB does not gain in low-pass noise; the table reports the figure, no test bounds it
MIN_ESTOI_GAIN = 0.03                   # ESTOI out - in:           0.0424      0.0523    0.0509     0.0611      0.0573
MAX_LEVEL_DB = 1.0                      # second-half level, dB:    -0.38       +0.19     +0.23      +0.30       +0.09
MAX_CREST_SPEECH = 6.5                  # crest of plain speech:    8.00 -> 5.57   (rule's output: 9.49 -> 8.58, 9.12 -> 8.45, 9.01 -> 8.31, 8.89 -> 6.74)
# (raw SIIB in, out, ESTOI in, out) measured with tests/drc_ref.py and oracle.siib / oracle.estoi
MEASURED = {
    ('ssn', -5.0, 'speech'): (28.44, 38.98, 0.2605, 0.3029),
    ('ssn', -5.0, 'rule'): (51.53, 63.65, 0.3321, 0.3845),
    ('pink', -5.0, 'rule'): (55.83, 69.78, 0.4015, 0.4524),
    ('white', 0.0, 'rule'): (84.25, 111.33, 0.6190, 0.6800),
    ('lowpass', -5.0, 'rule'): (105.49, 103.35, 0.3839, 0.4412),
}
# ---- the level step: the speech, then twice the speech at -20 dB; output over input level per half copy (2.1 s), dB
STEP_DB = -20.0
STEP_LAST_WINDOWS_WITHIN_DB = 2.0       # the last two windows; all six, measured: see STEP_MEASURED
STEP_MEASURED = (2.18, -0.38, 7.18, 3.53, -0.41, -1.18)
# ---- equivalence with the offline stage (equaliser off, ref_level = e0_ratio * max envelope): float32 equal in every sample,
# float64 within this of the peak (measured 5.8e-16: numpy's convolutions sum in another order than section 23's)
EQUIV_F64 = 1e-13
# ---- float32 output on the GPU: one rounding flip of the reference's peak (DESIGN.md section 14's bound)
OUT_BOUND = 2.0 ** -22
# ---- sensitivity: every a[i] one float64 ulp up or down at random, three seeds, the largest deviation over the seeds, measured with
# drc_ref on the inputs of the GPU parity shapes and rounded up to two digits (tests/test_drc_cpu.py measures them again).
# gain, level: relative, no sample or hop excluded (where the reference is exactly 0 - a stream's first hop - so is the other side).
# key: (shift of the speech in samples, hops)
SENS = {
    (0, 40): {'gain': 1.2e-15, 'level': 4.5e-16},      # shape (1, 40)
    (0, 264): {'gain': 1.3e-15, 'level': 4.5e-16},     # shape (3, 264), stream 0
    (5000, 264): {'gain': 1.3e-15, 'level': 4.5e-16},  # stream 1
    (10000, 264): {'gain': 1.4e-15, 'level': 4.5e-16}, # stream 2
}
SENS_INPUTS = tuple(SENS)
# The GPU bounds are 8 x these, per stream, and never more than SENS_CEILING: a GPU run differs from numpy in the roundings of log10
# and pow, where the experiment moves every magnitude; the factor covers the spread between seeds and those two functions.
GPU_FACTOR = 8.0
SENS_CEILING = 1e-12
GPU_SIIB_WITHIN, GPU_ESTOI_WITHIN = 0.005, 0.002       # the ssn row's figures on the GPU chain against the reference's
_CACHE = {}


def speech():
    """the toy speech, float64, 264 hops"""
    return C.far_and_near()[0]


def stream_input(shift, hops=264):
    """the speech circularly shifted by ``shift`` samples, float32, ``hops`` hops"""
    return np.roll(speech(), -shift)[:hops * HOP].astype(np.float32)


def ref_run(shift, hops):
    """stream_input through DrcRef(): computed once, shared, never changed"""
    key = ('r', shift, hops)
    if key not in _CACHE:
        _CACHE[key] = DrcRef().run(stream_input(shift, hops))
    return _CACHE[key]


def rel_dev(got, ref):
    """largest |got / ref - 1|; where ref is exactly 0 got must be too (else inf)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    z = ref == 0
    if np.any(got[z] != 0) or not np.all(np.isfinite(got)):
        return float('inf')
    return float(np.abs(got[~z] / ref[~z] - 1.0).max()) if np.any(~z) else 0.0


def flip_hook(seed):
    """a -> a with every element one float64 ulp up or down at random"""
    rng = np.random.default_rng(seed)

    def hook(a):
        up = rng.integers(0, 2, a.shape).astype(bool)
        return np.where(up, np.nextafter(a, np.inf), np.nextafter(a, 0.0))
    return hook


def sensitivity(x, base, seeds=(1, 2, 3)):
    """the all-flipped experiment on input x against the unperturbed run ``base`` -> the largest relative deviations over the seeds"""
    worst = {'gain': 0.0, 'level': 0.0}
    for seed in seeds:
        r = DrcRef(a_hook=flip_hook(seed)).run(x)
        for k in worst:
            worst[k] = max(worst[k], rel_dev(r[k], base[k]))
    return worst


def gpu_bound(key):
    return {k: min(GPU_FACTOR * v, SENS_CEILING) for k, v in SENS[key].items()}


# ------------------------------------------------------------------------------------------------ the table's rows
def row_input(kind, snr_db, what):
    """-> (speech, noise, the compressor's input) float64, 264 hops each"""
    sc = SK.scenario(kind, snr_db)
    sp, v = sc['speech'].astype(np.float64), sc['noise'].astype(np.float64)
    return sp, v, (sp if what == 'speech' else SK.ref_enhanced(kind, snr_db))


def to_rms_of(out, inp):
    out = np.asarray(out, dtype=np.float64)
    return out * np.sqrt(np.mean(inp * inp) / np.mean(out * out))


def score(sp, v, inp, out):
    """``out``: the compressor's output, realigned with ``inp`` -> dict: SIIB and ESTOI of input and of output (scaled to the input's
    rms), the second-half level of the unscaled output over the input's in dB, the crest factors of input and output"""
    out = np.asarray(out, dtype=np.float64)
    scaled = to_rms_of(out, inp)
    fi, fo = SK.figures(sp, v, inp), SK.figures(sp, v, scaled)
    h = len(inp) // 2
    return {'siib_in': fi[1], 'siib_out': fo[1], 'estoi_in': fi[3], 'estoi_out': fo[3],
            'level_db': float(10.0 * np.log10(np.sum(out[h:] ** 2) / np.sum(inp[h:] ** 2))), 'crest_in': S.crest(inp), 'crest_out': S.crest(scaled)}


def ref_row(kind, snr_db, what):
    """the row through drc_ref: computed once, shared, never changed"""
    key = ('row', kind, snr_db, what)
    if key not in _CACHE:
        sp, v, inp = row_input(kind, snr_db, what)
        _CACHE[key] = score(sp, v, inp, compress_stream(inp.astype(np.float32)))
    return _CACHE[key]


def step_signal():
    """the speech, then twice the speech at -20 dB, float32"""
    sp = speech()
    q = sp * 10.0 ** (STEP_DB / 20.0)
    return np.concatenate([sp, q, q]).astype(np.float32)


def step_levels(x, out):
    """output over input level of each half of each of the three copies (2.112 s windows), dB (``out`` realigned with ``x``)"""
    w = len(x) // 6
    x, out = np.asarray(x, dtype=np.float64), np.asarray(out, dtype=np.float64)
    return [float(10.0 * np.log10(np.sum(out[i * w:(i + 1) * w] ** 2) / np.sum(x[i * w:(i + 1) * w] ** 2))) for i in range(6)]
