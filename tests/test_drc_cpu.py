"""CPU: tests/drc_ref.py - the float64 numpy restatement of DESIGN.md section 23, the causal dynamic range compressor - on its own: its
equivalence with the offline stage of section 11 (tests/ssdrc_ref.py), the figures of section 23's table with the oracle's SIIB and
ESTOI, the level step, silence, its own hop-grouping invariance, the sensitivity experiment the GPU bounds stand on, and the argument
checks of nele_gan_amd/drc.py's classes and command line, which run before any device is touched."""
import numpy as np
import pytest

import drc_cases as K
import ssdrc_ref as S
from drc_ref import HOP, DrcRef, compress_stream, factor, hop_sum


def test_fixed_level_and_no_equaliser_is_the_offline_stage():
    """the toy speech (264 hops) plus one zero hop: from hop 1 on the output is float32(ssdrc_ref.compress) in every sample"""
    s = np.concatenate([K.speech().astype(np.float32), np.zeros(HOP, np.float32)])
    level = S.Params().e0_ratio * S.envelope(s.astype(np.float64)).max()
    r = DrcRef(equalise=False, ref_level=level).run(s)
    off = S.compress(s.astype(np.float64))[0][:264 * HOP]
    differ = int((r['out'][HOP:] != off.astype(np.float32)).sum())
    dev = float(np.abs(r['out64'][HOP:] - off).max() / np.abs(off).max())
    print('%d of %d float32 samples differ; float64: %.2g of the peak (bound %.0e)' % (differ, off.size, dev, K.EQUIV_F64))
    assert off.size == 67584 and differ == 0 and dev <= K.EQUIV_F64
    assert not r['out'][:HOP].any() and np.all(r['level'][1:] == level) and r['level'][0] == 0
    # the smoothed envelope too, from the stream's first sample on (the magnitude is zero before the stream's start, as offline)
    e_hat = S.compress(s.astype(np.float64))[1][:264 * HOP]
    assert np.abs(r['ehat'][HOP:] - e_hat).max() <= 1e-13 * e_hat.max()


@pytest.mark.parametrize('kind,snr_db,what', K.ROWS)
def test_figures_of_the_table(kind, snr_db, what):
    r = K.ref_row(kind, snr_db, what)
    ratio, gain = r['siib_out'] / r['siib_in'], r['estoi_out'] - r['estoi_in']
    print('%s %g dB, %s: SIIB %.2f -> %.2f (x %.3f), ESTOI %.4f -> %.4f (+%.4f), level %+.2f dB, crest %.2f -> %.2f'
          % (kind, snr_db, what, r['siib_in'], r['siib_out'], ratio, r['estoi_in'], r['estoi_out'], gain, r['level_db'], r['crest_in'], r['crest_out']))
    if (kind, snr_db, what) in K.SIIB_BOUND_ROWS:
        assert ratio >= K.MIN_SIIB_RATIO
    assert gain >= K.MIN_ESTOI_GAIN
    assert abs(r['level_db']) <= K.MAX_LEVEL_DB
    if what == 'speech':
        assert r['crest_out'] <= K.MAX_CREST_SPEECH < r['crest_in']
    m = K.MEASURED[(kind, snr_db, what)]                  # the record beside the bounds is what this machine measures
    assert np.allclose([r['siib_in'], r['siib_out']], m[:2], rtol=2e-3) and np.allclose([r['estoi_in'], r['estoi_out']], m[2:], atol=2e-4)


def test_level_step():
    """the speech, then twice the speech at -20 dB: the level is back within 2 dB in the last copy; the copy right behind the drop comes
    out too loud while M decays (DESIGN.md section 23 says so)"""
    x = K.step_signal()
    lv = K.step_levels(x, compress_stream(x))
    print('output over input level per half copy, dB: ' + ', '.join('%+.2f' % v for v in lv))
    assert len(lv) == 6 and all(abs(v) <= K.STEP_LAST_WINDOWS_WITHIN_DB for v in lv[4:])
    assert np.allclose(lv, K.STEP_MEASURED, atol=0.02)


def test_silence_then_speech_stays_finite():
    ref = DrcRef()
    r = ref.run(np.zeros(40 * HOP, np.float32))
    assert all(np.all(r[k] == 0) for k in ('out', 'out64', 'level', 'ehat')) and np.all(r['gain'][HOP:] == 1) and not r['gain'][:HOP].any()
    st = ref.state()
    assert all(np.all(np.isfinite(v)) for v in st.values()) and st['count'] == 2 and st['g_prev'] == 1.0 and st['M'] == 0.0
    r = ref.run(K.stream_input(0, 40))
    assert all(np.all(np.isfinite(v)) for v in r.values()) and r['out'].any()
    assert all(np.all(np.isfinite(v)) for v in ref.state().values())


def test_hop_grouping_is_bitwise_in_the_reference():
    x = K.stream_input(5000, 40)
    whole = K.ref_run(5000, 40)
    for group in (1, 7):
        ref = DrcRef()
        parts = [ref.run(x[a:a + group * HOP]) for a in range(0, len(x), group * HOP)]
        for k in whole:
            assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k]), (group, k)
    assert hop_sum(np.ones(HOP)) == 256.0 and factor(4.0) == float(np.exp(-0.004))


@pytest.mark.parametrize('shift,hops', K.SENS_INPUTS)
def test_sensitivity_to_one_ulp_of_every_magnitude(shift, hops):
    """the basis of the GPU bounds: measured again here, held under what drc_cases.py records (and not far under: the record is honest)"""
    got = K.sensitivity(K.stream_input(shift, hops), K.ref_run(shift, hops))
    print(shift, hops, got)
    for k, v in K.SENS[(shift, hops)].items():
        assert 0.5 * v <= got[k] <= v, (k, got[k], v)
        assert K.gpu_bound((shift, hops))[k] == K.GPU_FACTOR * v <= K.SENS_CEILING


def test_python_classes_and_command_line_reject_bad_arguments_before_touching_a_device():
    from nele_gan_amd import drc as D
    from nele_gan_amd.ssdrc import SsdrcParams
    for kw, what in (({'streams': 0}, 'streams'), ({'tau_peak': 0.0}, 'tau_peak'), ({'tau_peak': float('nan')}, 'tau_peak'),
                     ({'tau_energy': -1.0}, 'tau_energy'), ({'tau_energy': 1e300}, 'tau_energy'), ({'params': object()}, 'SsdrcParams'),
                     ({'params': SsdrcParams(attack=1.0)}, 'attack'), ({'params': SsdrcParams(release=-0.1)}, 'release'),
                     ({'params': SsdrcParams(e0_ratio=0.0)}, 'e0_ratio'), ({'params': SsdrcParams(knots=((0.0, 0.0),))}, 'knots'),
                     ({'params': SsdrcParams(knots=((0.0, 0.0), (-1.0, 0.0)))}, 'knots'),
                     ({'params': SsdrcParams(knots=((0.0, float('inf')), (1.0, 0.0)))}, 'knots'),
                     ({'streams': 2, 'ref_level': [0.1]}, 'ref_level'), ({'ref_level': [-0.1]}, 'ref_level'),
                     ({'ref_level': [float('nan')]}, 'ref_level')):
        with pytest.raises(ValueError, match=what):
            D.StreamCompressor(**dict({'streams': 1}, **kw))

    class Stub:
        def __init__(self, S):
            self.S = S
    with pytest.raises(ValueError, match='streams'):
        D.CompressedEnhancer(Stub(2), Stub(3))
    assert D.hop_factor(4.0, 'tau_peak') == factor(4.0) and D.hop_factor(1.0, 'tau_energy') == factor(1.0)
    assert 'ECHO LOOP MUST SEE THE COMPRESSED SIGNAL' in D.__doc__
    for argv in (['--in', 'a.wav'], ['--out', 'b.wav'], ['--in', 'a.wav', '--out', 'b.wav', '--tau-peak', '0'],
                 ['--in', 'a.wav', '--out', 'b.wav', '--tau-energy', '-2'], ['--in', 'a.wav', '--out', 'b.wav', '--tau-peak', 'nan']):
        with pytest.raises(SystemExit):
            D.main(argv)
