"""CPU: the running ESTOI's reference (tests/monitor_ref.py) and cases (tests/monitor_cases.py) before anything runs on a GPU - the
premise that lets the device test compare gate decisions exactly, the tie of the streaming measure to oracle/estoi.py, its invariance
to the hop grouping, the constants of DESIGN.md section 27, and the Python classes' argument checks, which precede any GPU call.

Measured: the streaming segment values differ from oracle_stages()['dseg'] by at most 2.8e-16 on the three oracle cases (bound 1e-9);
the nearest frame is 0.0877 dB from the gate (gapped_boost)."""
import numpy as np
import pytest

import estoi_cases as EC
import monitor_cases as C
import monitor_ref as R

DSEG_ABS = 1e-9                  # the project's bound on a segment value (tests/test_estoi_stages_gpu.py)


def test_the_resamplers_constants_follow_from_the_formula():
    """output m is final once input floor((8 m + 290) / 5) has arrived: 160 (h + 1) - 36 samples after hop h, and a hop's oldest
    input lies 115 samples before it"""
    for h in range(12):
        assert R.final_samples(h + 1) == 160 * (h + 1) - 36
    m = R.Monitor()
    assert len(m.plan) == 160 and min(lo for lo, _, _ in m.plan) == R.HIST - 115 and max(hi for _, hi, _ in m.plan) <= R.HIST + 255
    assert {len(t) for _, _, t in m.plan} == {116, 117} and abs(sum(t.sum() for _, _, t in m.plan) / 160 - 1.0) < 1e-12
    assert len(R.taps()) == 581 and abs(R.taps().sum() - 5.0) < 1e-12


def test_every_final_sample_equals_the_offline_resampling_of_the_whole_stream():
    x, _ = C.case('steady')
    whole = EC.E.resample_16k_to_10k(x.astype(np.float64))
    m = R.Monitor()
    hist, worst = np.zeros(R.HIST), 0.0
    for h in range(len(x) // R.HOP):
        before = m.tail.shape[1] + 128 * int(m.s[R.SEEN])
        m.hop(x[h * R.HOP:(h + 1) * R.HOP])
        assert m.tail.shape[1] + 128 * int(m.s[R.SEEN]) == 160 * (h + 1) - 36 and before == max(160 * h - 36, 0)
        xin = np.concatenate([hist, x[h * R.HOP:(h + 1) * R.HOP].astype(np.float64)])
        new = np.array([np.dot(xin[lo:hi], t) for lo, hi, t in m.plan])[36 if h == 0 else 0:]
        worst = max(worst, np.max(np.abs(new - whole[max(160 * h - 36, 0):160 * h + 124])))
        hist = xin[R.HOP:]
    print('10 kHz samples of the stream against the offline resampling: max difference %.3g' % worst)
    assert worst < 1e-15                                                          # signals of amplitude 0.1: rounding of a 117-term sum
    # and a prefix of the stream differs from the whole in its last 35 outputs only
    part = EC.E.resample_16k_to_10k(x[:20 * R.HOP].astype(np.float64))
    differ = np.flatnonzero(np.abs(part - whole[:len(part)]) > 1e-15)
    assert len(part) == 3200 and differ.min() >= 3200 - 36
    # the frames the stream saw are the offline signal's: the energies agree to rounding
    en = EC.oracle_stages(*C.case('steady'))['en']
    mine = np.array([f[0] for f in C.reference('steady')['frames']])
    assert len(mine) == 48 and np.max(np.abs(mine - en[:48])) < 1e-9 and len(whole) == 6400


@pytest.mark.parametrize('name', C.NAMES)
def test_no_frame_of_any_case_lies_at_the_causal_gate(name):
    ref = C.reference(name)
    print('%s: %d frames, %d kept, nearest %.4g dB from the gate' % (name, ref['stats'][R.SEEN], ref['stats'][R.KEPT], C.margin(ref['frames'])))
    assert C.margin(ref['frames']) > EC.GATE_MARGIN_DB
    assert ref['nseg'].max() <= 2 and not np.isnan(ref['stats']).any()
    if name in C.EXPECTED:
        hops, seen, kept = C.EXPECTED[name]
        assert (len(C.case(name)[0]) // R.HOP, ref['stats'][R.SEEN], ref['stats'][R.KEPT]) == (hops, seen, kept)


@pytest.mark.parametrize('name', C.ORACLE_NAMES)
def test_the_streaming_segments_are_estois(name):
    """the causal gate equals the global one on every frame, the segment values are oracle_stages()['dseg'][:n] within DSEG_ABS, n one
    kept frame and the resampler's 36 samples behind the whole-signal count, and the cumulative reading is their mean"""
    x, y = C.case(name)
    ref, o = C.reference(name), EC.oracle_stages(x, y)
    nf = len(ref['frames'])
    assert nf == len(o['en']) - (1 if name == 'steady' else 0)
    assert np.array_equal(np.array([k for _, _, k in ref['frames']]), np.isin(np.arange(nf), o['keep']))
    v, n = ref['values'], len(ref['values'])
    kept = int(ref['stats'][R.KEPT])
    assert n == kept - 30 and 0 < n <= len(o['dseg']) - 1 and not np.isnan(v).any()
    print('%s: %d segments, max |d - dseg| = %.3g' % (name, n, np.max(np.abs(v - o['dseg'][:n]))))
    assert np.max(np.abs(v - o['dseg'][:n])) <= DSEG_ABS
    s = ref['stats']
    assert s[R.COUNT] == n and s[R.SKIPPED] == 0 and abs(s[R.SUM] / s[R.COUNT] - np.mean(o['dseg'][:n])) <= DSEG_ABS and s[R.LAST] == v[-1]
    assert abs(s[R.SUM] / s[R.COUNT] - o['raw']) < 0.02                           # and so near the offline score


def test_quiet_start_tells_the_causal_gate_from_the_global_one():
    x, y = C.case('quiet_start')
    ref, o = C.reference('quiet_start'), EC.oracle_stages(x, y)
    kept = np.array([k for _, _, k in ref['frames']])
    glob = np.isin(np.arange(len(kept)), o['keep'])
    assert kept.all() and not glob[:30].any() and glob[45:].all() and kept.sum() - glob.sum() >= 30


def test_the_special_cases_do_what_the_design_says():
    s = C.reference('silence')['stats']
    assert s[R.COUNT] == 0 and s[R.SUM] == 0 and s[R.LAST] == 0 and s[R.SMOOTH] == 0 and s[R.SKIPPED] == s[R.KEPT] - 30 > 0 and s[R.KEPT] == s[R.SEEN]
    assert np.isnan(C.reference('silence')['values']).all() and abs(s[R.M] - 20 * np.log10(EC.E.EPS)) < 1e-9
    g = C.reference('long_gap')
    dropped = np.array([not k for _, _, k in g['frames']])
    runs = np.flatnonzero(np.diff(np.concatenate([[0], dropped.astype(int), [0]])))
    assert len(runs) == 2 and runs[1] - runs[0] >= 40 and g['stats'][R.SKIPPED] == 0 and g['stats'][R.COUNT] == g['stats'][R.KEPT] - 30
    steady = C.reference('nan_both')['stats'][R.SEEN]
    d, b = C.reference('nan_deg'), C.reference('nan_both')
    assert d['stats'][R.KEPT] == d['stats'][R.SEEN] == steady and 25 <= d['stats'][R.SKIPPED] <= 36 and np.isfinite(d['values'][-30:]).all()
    assert 3 <= b['stats'][R.SEEN] - b['stats'][R.KEPT] <= 5 and b['stats'][R.SKIPPED] == 0 and not np.isnan(b['values']).any()
    assert np.array_equal(d['values'][-20:], C.reference('nan_both')['values'][-20:]) or np.isfinite(d['values'][-20:]).all()


@pytest.mark.parametrize('lag', [0, 2])
def test_the_reference_does_not_depend_on_the_hop_grouping_and_lag_shifts_the_start(lag):
    """one Monitor fed hop by hop is the definition; run() cut in two calls on one object gives the same, and with lag the measure is
    that of (ref[:-lag hops], deg[lag hops:]) at lag 0"""
    x, y = C.case('quiet_start')
    whole = R.run(x, y, lag=lag, alpha=C.ALPHA)
    mon = R.Monitor(lag, C.ALPHA)
    cut = 23 * R.HOP
    a = R.run(x[:cut], y[:cut], mon=mon)
    b = R.run(x[cut:], y[cut:], mon=mon)
    assert np.array_equal(np.concatenate([a['seg'], b['seg']]), whole['seg'], equal_nan=True) and np.array_equal(b['stats'], whole['stats'])
    if lag:
        zero = R.run(x[:-lag * R.HOP], y[lag * R.HOP:], alpha=C.ALPHA)
        assert np.array_equal(zero['seg'], whole['seg'][lag:], equal_nan=True) and np.array_equal(zero['stats'], whole['stats'])
        assert not whole['nseg'][:lag].any()


def test_the_smoothing_factor_and_the_map_are_the_designs():
    from nele_gan_amd import metrics
    from nele_gan_amd.monitor import map_estoi, smoothing_factor
    import torch
    assert smoothing_factor(1.0) == R.alpha_of(1.0) == float(1.0 - np.exp(-0.0128)) and smoothing_factor(0.25) == C.ALPHA
    d = np.array([-0.2, 0.0, 0.25, 0.6, 1.0])
    assert np.allclose(map_estoi(torch.from_numpy(d)).numpy(), metrics.mapping_ESTOI_harvard(d), rtol=0, atol=1e-15)


def test_the_python_classes_reject_bad_parameters_before_any_gpu_call():
    from nele_gan_amd.monitor import MonitoredEnhancer, StreamMonitor, lag_of, smoothing_factor
    for kw in ({'streams': 0}, {'lag': -1}, {'lag': 5}, {'lag': 1.5}, {'lag': True}, {'time_constant': 0.0}, {'time_constant': -1.0},
               {'time_constant': float('nan')}, {'time_constant': float('inf')}, {'time_constant': 1e30}):
        with pytest.raises(ValueError):
            StreamMonitor(**dict({'streams': 2}, **kw))
    with pytest.raises(ValueError):
        smoothing_factor(0.0)

    class Inner:                                                                   # stands for an enhancer: never called
        def __init__(self, S, **kw):
            self.S = S
            self.__dict__.update(kw)

    class Mon:
        def __init__(self, S, lag):
            self.S, self.lag = S, lag

    assert lag_of(Inner(2)) == 1 and lag_of(Inner(2, drc=object())) == 2 and lag_of(Inner(2, drc=object(), lag_hops=3)) == 3
    for inner, mon, base in ((Inner(2), Mon(3, 1), None), (Inner(2), Mon(2, 2), None), (Inner(2, drc=1), Mon(2, 1), None),
                             (Inner(2, lag_hops=3), Mon(2, 3), Mon(2, 2)), (Inner(2), Mon(2, 1), Mon(4, 1))):
        with pytest.raises(ValueError):
            MonitoredEnhancer(inner, mon, base)
    chain = MonitoredEnhancer(Inner(2, lag_hops=3), Mon(2, 3), Mon(2, 3))
    assert chain.lag_hops == 3 and chain.S == 2
    with pytest.raises(ValueError):
        MonitoredEnhancer(Inner(2), Mon(2, 1)).benefit()
