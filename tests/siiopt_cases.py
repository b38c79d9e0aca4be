"""The scenarios and every bound shared by tests/test_siiopt_cpu.py and tests/test_siiopt_gpu.py: the toy far end
of tests/aec_cases.py at rms 0.03 as the speech, stationary synthetic noise of four colours (``default_rng(7)``) at a stated SNR over the
whole signal, the oracle's features, and tests/siiopt_ref.py in the generator's place with the utterance-level normalisation, the
oracle's resynthesis and the final rms 0.03.  Each bound has the value measured with the reference beside it."""
import numpy as np
from scipy.signal import butter, lfilter

import aec_cases as C
import siiopt_ref as R
from ns_cases import PINK_A, PINK_B

RMS = 0.03
# (noise, SNR dB): the four rows of DESIGN.md section 22's table
SCENARIOS = (('ssn', -5.0), ('pink', -5.0), ('white', 0.0), ('lowpass', -5.0))

# ---- bounds of the figures at strength 0.5       measured with siiopt_ref:   ssn -5 dB   pink -5 dB   white 0 dB   low-pass -5 dB
MIN_SIIB_RATIO = {'ssn': 1.3, 'pink': 1.3, 'white': 1.3, 'lowpass': 1.05}   # raw SIIB after / before (see MEASURED below)
MIN_ESTOI_GAIN = 0.01                                                        # ESTOI after - before (see MEASURED below)
# (raw SIIB before, after, ESTOI before, after), measured with tests/siiopt_ref.py and oracle.siib / oracle.estoi
MEASURED = {
    'ssn': (28.44, 51.53, 0.2605, 0.3321),          # x 1.812   (strength 1: x 1.910, ESTOI 0.2882)
    'pink': (33.26, 55.83, 0.3247, 0.4015),         # x 1.679   (strength 1: x 1.693, ESTOI 0.3435)
    'white': (58.67, 84.25, 0.5149, 0.6190),        # x 1.436   (strength 1: x 1.479, ESTOI 0.5757)
    'lowpass': (89.33, 105.5, 0.3623, 0.3839),      # x 1.181   (strength 1: x 1.118, ESTOI 0.3311: below unprocessed)
}
# ---- the GPU tolerance: relative, on every mask value, none excluded.  Its basis is the sensitivity experiment of test_siiopt_cpu.py:
# the reference with its three sums taken in reversed band order moves no float32 mask value of the parity inputs by more than an eighth
# of this (measured: 0 - no float32 mask value of the four scenarios differs at all).
GPU_RTOL = 1e-6
MAX_REVERSED_ORDER_DEVIATION = GPU_RTOL / 8
# resynthesised signals against oracle.features.sp_to_wav: the tolerance of gain_istft's own tests (tests/test_features_gpu.py)
WAV_ATOL = 2e-5
_CACHE = {}


def noise(kind, n):
    v = np.random.default_rng(7).standard_normal(n)
    if kind == 'ssn':
        return lfilter([1.0], [1.0, -0.9], v)
    if kind == 'pink':
        return lfilter(PINK_B, PINK_A, v)
    if kind == 'lowpass':
        b, a = butter(4, 1000.0 / 8000.0)
        return lfilter(b, a, v)
    assert kind == 'white'
    return v


def scenario(kind, snr_db):
    """-> dict: speech (rms 0.03), noise (scaled to the SNR over the whole signal), float32, 264 hops each"""
    key = ('s', kind, snr_db)
    if key not in _CACHE:
        speech, _ = C.far_and_near()
        speech = speech * (RMS / np.sqrt(np.mean(speech * speech)))
        v = noise(kind, len(speech))
        v = v * np.sqrt(np.sum(speech * speech) / (np.sum(v * v) * 10.0 ** (snr_db / 10.0)))
        _CACHE[key] = {'speech': speech.astype(np.float32), 'noise': v.astype(np.float32)}
    return _CACHE[key]


def features(kind, snr_db):
    """the oracle's features of the scenario: cb, nb [T, 64] float32, mag, phase [257, T] - computed once, shared, never changed"""
    key = ('f', kind, snr_db)
    if key not in _CACHE:
        from oracle import features as F
        s = scenario(kind, snr_db)
        cb, mag, phase = F.sp_and_phase_speech(s['speech'], 1.0 / 6)
        nb, _, _ = F.sp_and_phase_noise(s['noise'], 1.0 / 6)
        _CACHE[key] = {'cb': np.ascontiguousarray(cb, dtype=np.float32), 'nb': np.ascontiguousarray(nb, dtype=np.float32), 'mag': mag,
                       'phase': phase}
    return _CACHE[key]


def ref_mask(kind, snr_db, strength=0.5, lam=R.LAMBDA):
    key = ('m', kind, snr_db, strength, lam)
    if key not in _CACHE:
        f = features(kind, snr_db)
        _CACHE[key] = R.mask(f['cb'], f['nb'], strength=strength, lam=lam)
    return _CACHE[key]


def ref_enhanced(kind, snr_db, strength=0.5):
    """the reference chain's output at rms 0.03, float64 [264 * 256]"""
    key = ('e', kind, snr_db, strength)
    if key not in _CACHE:
        from oracle import features as F
        f = features(kind, snr_db)
        a2 = R.alpha2_utterance(ref_mask(kind, snr_db, strength), f['cb'])
        enh = np.asarray(F.sp_to_wav(a2, f['mag'], f['phase']), dtype=np.float64)
        _CACHE[key] = enh * (RMS / np.sqrt(np.mean(enh * enh)))
    return _CACHE[key]


def figures(speech, noise, enh):
    """-> (raw SIIB before, after, ESTOI before, after) of ``enh`` played in ``noise``, with oracle.siib / oracle.estoi"""
    from oracle import estoi, siib
    x, v, y = (np.asarray(a, dtype=np.float64) for a in (speech, noise, enh))
    n = min(len(x), len(y))
    x, v, y = x[:n], v[:n], y[:n]
    return (siib.siib_wrapper(x, x + v, norm=False), siib.siib_wrapper(x, y + v, norm=False),
            estoi.estoi_wrapper(x, x + v, norm=False), estoi.estoi_wrapper(x, y + v, norm=False))


def parity_inputs():
    """the (cb, nb) [T, 64] rows of the GPU parity shapes: the four scenarios' features, 264 frames each (the 265th is dropped)"""
    return [(features(k, s)['cb'][:264], features(k, s)['nb'][:264]) for k, s in SCENARIOS]
