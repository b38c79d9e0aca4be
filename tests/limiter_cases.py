"""The inputs and every bound shared by tests/test_limiter_cpu.py and tests/test_limiter_gpu.py: the toy far end
of tests/aec_cases.py as the speech, scaled so that its peak stands `over` dB above the ceiling, tones that start abruptly with the
stream, a 7.3 kHz burst, the 16 -> 48 kHz conversion of tests/resample_ref.py as the up-converter behind the limiter, and the scenarios
of tests/siiopt_cases.py with the oracle's SIIB and ESTOI.  Each bound has the value measured with tests/limiter_ref.py beside it."""
import numpy as np

import aec_cases as C
import resample_ref as RR
import siiopt_cases as SK
from limiter_ref import CEILING, HOP, LimRef, limit_stream

OVERS = (-3.0, 6.0, 12.0)                                  # dB of the speech's peak over the ceiling: transparent, moderate, heavy
TONES = (2611.0, 4037.0, 5333.0)                           # Hz
TONE_HOPS = 12
# ---- inter-sample control: the largest |sample| of the limited output behind the 16 -> 48 kHz conversion (quality 'high': 32 zero
# crossings, Kaiser 12), over the ceiling.  Measured with tests/limiter_ref.py, (with the taps, without them); the bound is the value
# with the taps + TRUE_PEAK_ROOM: room for another resampler's ripple, not for a regression.
TRUE_PEAK_ROOM = 0.005
MEASURED_TRUE_PEAK = {
    'speech +12': (1.0187, 1.0412),
    'tone 2611': (0.9985, 1.0558),
    'tone 4037': (1.0294, 1.0964),
    'tone 5333': (1.0195, 1.1056),
}
# ---- the limiter against scaling the signal down until it fits, both at a peak `drive` dB above the ceiling before they act:
# (raw SIIB limiter, scaled, ESTOI limiter, scaled), measured with tests/limiter_ref.py and oracle.siib / oracle.estoi.  The bound on
# the SIIB ratio is SIIB_MARGIN of the measured one - the margin DESIGN.md section 23's rows leave between their ratios and their bounds.
SIIB_MARGIN = 0.85
FIT_ROWS = (('ssn', -5.0, 6.0), ('ssn', -5.0, 12.0), ('white', 0.0, 6.0), ('white', 0.0, 12.0))
MEASURED = {
    ('ssn', -5.0, 6.0): (27.23, 9.33, 0.2482, 0.0972),        # ratio 2.92; a hard clip at the ceiling: 28.28 / 0.2593
    ('ssn', -5.0, 12.0): (18.42, 3.80, 0.1824, 0.0232),       # 4.85; 25.38 / 0.2338
    ('white', 0.0, 6.0): (57.37, 34.94, 0.5059, 0.3561),      # 1.64; 58.27 / 0.5137
    ('white', 0.0, 12.0): (49.79, 18.62, 0.4574, 0.2040),     # 2.67; 54.63 / 0.4951
}
_CACHE = {}


def toy():
    """the toy speech, float64, 264 hops"""
    return C.far_and_near()[0]


def speech(over_db, shift=0, hops=264, ceiling=CEILING):
    """the first ``hops`` hops of the speech circularly shifted by ``shift`` samples, scaled so that the peak of those hops is
    ``over_db`` dB above the ceiling, float32"""
    s = np.roll(toy(), -shift)[:hops * HOP]
    return (s * (ceiling * 10.0 ** (over_db / 20.0) / np.abs(s).max())).astype(np.float32)


def tone(freq, over_db=6.0, hops=TONE_HOPS, ceiling=CEILING):
    """a cosine that starts at full amplitude with the stream's first sample, ``over_db`` dB above the ceiling, float32"""
    n = np.arange(hops * HOP)
    return (ceiling * 10.0 ** (over_db / 20.0) * np.cos(2.0 * np.pi * freq * n / 16000.0)).astype(np.float32)


def burst(over_db=6.0, hops=TONE_HOPS, ceiling=CEILING):
    """silence, 400 samples of 7.3 kHz under a Hann envelope from sample 700 on, silence: near the band's edge the samples miss most
    of the waveform's peaks"""
    x = np.zeros(hops * HOP)
    n = np.arange(400)
    x[700:1100] = ceiling * 10.0 ** (over_db / 20.0) * np.sin(2.0 * np.pi * 7300.0 * n / 16000.0) * (0.5 - 0.5 * np.cos(2.0 * np.pi * n / 399.0))
    return x.astype(np.float32)


def ref_run(key, **kw):
    """a named input through LimRef(**kw): computed once, shared, never changed.  key: ('speech', over, shift, hops), ('tone', freq),
    ('burst',)"""
    k = (key, tuple(sorted(kw.items())))
    if k not in _CACHE:
        _CACHE[k] = LimRef(**kw).run(named(key))
    return _CACHE[k]


def named(key):
    if key[0] == 'speech':
        return speech(*key[1:])
    return tone(key[1]) if key[0] == 'tone' else burst()


def true_peak_inputs():
    return dict({'speech +12': speech(12.0)}, **{'tone %d' % f: tone(f) for f in TONES})


def peak_at_48k(out, ceiling=CEILING):
    """the largest |sample| of ``out`` behind the 16 -> 48 kHz conversion, over the ceiling"""
    zeros, beta = RR.PRESETS['high']
    return float(np.abs(RR.scipy_resample(np.asarray(out, dtype=np.float64), 3, 1, RR.taps(3, 1, zeros, beta))).max() / ceiling)


# ------------------------------------------------------------------------------------------------ the limiter against scaled-to-fit
def fit_row(kind, snr_db, drive_db, how='limiter', ceiling=CEILING):
    """The scenario's speech, played at a peak ``drive_db`` dB above the ceiling, brought under it by ``how`` - 'limiter' (LimRef), 'scaled'
    (turned down until the peak fits) or 'clip' - in the scenario's noise -> (raw SIIB, ESTOI).  The noise is as loud
    as the scenario has it against the speech at that peak, whatever ``how`` does: the room does not turn down with the loudspeaker."""
    k = ('fit', kind, snr_db, drive_db, how)
    if k not in _CACHE:
        sc = SK.scenario(kind, snr_db)
        sp, v = sc['speech'].astype(np.float64), sc['noise'].astype(np.float64)
        unit = ceiling / np.abs(sp).max()                                # the scale at which the clean speech just fits
        loud = (sp * unit * 10.0 ** (drive_db / 20.0)).astype(np.float32)
        if how == 'limiter':
            played = limit_stream(loud)['out'].astype(np.float64)
        elif how == 'scaled':
            played = loud.astype(np.float64) * 10.0 ** (-drive_db / 20.0)
        else:
            played = np.clip(loud.astype(np.float64), -ceiling, ceiling)
        noise = v * unit * 10.0 ** (drive_db / 20.0)                     # the room's noise: as loud as the scenario has it against `loud`
        f = SK.figures(sp, noise, played)
        _CACHE[k] = (f[1], f[3])
    return _CACHE[k]
