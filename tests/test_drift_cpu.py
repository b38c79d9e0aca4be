"""CPU: the clock-drift compensator's C ABI (nele_drift_* of include/nele_hip_ext2.h: state-size arithmetic, bad arguments rejected
without a GPU; the header and the binding as a whole: tests/test_abi_ext2_cpu.py), the Python classes' refusals,
DriftTrackedEchoCanceller's bookkeeping on stubs, and the numpy reference tests/drift_ref.py on its own against DESIGN.md section 19:
the table, the warp on sinusoids, the ring's limits, the closed loop at +100 and 0 ppm, on an echo-free microphone and on a silent
far end, the snap, and the perturbation figure from which tests/test_drift_gpu.py's bound on tau derives."""
import ctypes

import numpy as np
import pytest

import drift_cases as DC
from aec_ref import AecRef
from drift_ref import HOP, MAX_RATE, TAU_MIN, DriftRef, table, tau_max

LL = ctypes.c_longlong


def _lib():
    from nele_gan_amd import _lib
    return _lib.lib


def _err():
    return _lib().nele_last_error_string()


# ------------------------------------------------------------------------------------------------------------------------ the C ABI
def test_state_bytes_are_a_header_the_table_and_one_record_per_stream():
    lib = _lib()
    for Q in (2, 3, 8, 32, 64):
        rec = lib.nele_drift_stream_record_bytes(Q)
        # the ring of Q + 4 hops (float32), u_prev, S_d, S_u (257 float64 each), C_f, C_s (257 complex128 each); under 2 KB beside them
        need = (Q + 4) * 256 * 4 + 256 * 4 + 2 * 257 * 8 + 2 * 256 * 16
        assert need <= rec <= need + 2048 and rec % 256 == 0, Q
        header = lib.nele_drift_state_bytes(1, Q) - rec
        assert 65 * 64 * 8 < header <= 65 * 64 * 8 + 4096 and header % 256 == 0
        for B in (1, 2, 16, 4096, 1 << 20):
            assert lib.nele_drift_state_bytes(B, Q) == header + B * rec
    for B, Q in ((0, 8), (-1, 8), ((1 << 20) + 1, 8), (4, 1), (4, 65), (4, 0)):
        assert lib.nele_drift_state_bytes(B, Q) == -1
    for Q in (1, 65, -3):
        assert lib.nele_drift_stream_record_bytes(Q) == -1


def test_bad_arguments_are_rejected_without_a_gpu():
    lib = _lib()
    B, Q = 4, 8
    need = lib.nele_drift_state_bytes(B, Q)
    fake = ctypes.c_void_p(1 << 20)                                 # never dereferenced: every call below fails its checks first
    odd = ctypes.c_void_p((1 << 20) + 16)
    nan, inf = float('nan'), float('inf')

    def hop(state=fake, nbytes=need, S=B, blocks=Q, mic=fake, played=fake, base=fake, nh=1, lf=0.9, ls=0.99, kp=0.02, ki=5e-4, aligned=fake):
        return lib.nele_drift_hop(state, LL(nbytes), S, blocks, mic, played, base, None, None, nh, lf, ls, kp, ki, aligned, None, None)

    cases = [
        (lambda: hop(state=None), b'nele_drift_hop', b'state'),
        (lambda: hop(nbytes=need - 1), b'nele_drift_hop', b'nele_drift_state_bytes'),
        (lambda: hop(S=0), b'nele_drift_hop', b'max_streams'),
        (lambda: hop(S=(1 << 20) + 1, nbytes=1 << 50), b'nele_drift_hop', b'max_streams'),
        (lambda: hop(blocks=1), b'nele_drift_hop', b'blocks'),
        (lambda: hop(blocks=65, nbytes=1 << 40), b'nele_drift_hop', b'blocks'),
        (lambda: hop(state=odd), b'nele_drift_hop', b'256-byte aligned'),
        (lambda: hop(mic=None), b'nele_drift_hop', b'mic'),
        (lambda: hop(played=None), b'nele_drift_hop', b'played'),
        (lambda: hop(base=None), b'nele_drift_hop', b'base_hops'),
        (lambda: hop(aligned=None), b'nele_drift_hop', b'aligned'),
        (lambda: hop(nh=0), b'nele_drift_hop', b'nh'),
        (lambda: hop(nh=(1 << 20) + 1), b'nele_drift_hop', b'nh'),
        (lambda: hop(lf=0.0), b'nele_drift_hop', b'lam_fast'),
        (lambda: hop(lf=1.0), b'nele_drift_hop', b'lam_fast'),
        (lambda: hop(lf=nan), b'nele_drift_hop', b'lam_fast'),
        (lambda: hop(ls=0.9), b'nele_drift_hop', b'lam_slow'),
        (lambda: hop(ls=0.5), b'nele_drift_hop', b'lam_slow'),
        (lambda: hop(ls=1.0), b'nele_drift_hop', b'lam_slow'),
        (lambda: hop(ls=nan), b'nele_drift_hop', b'lam_slow'),
        (lambda: hop(kp=-1e-9), b'nele_drift_hop', b'kp'),
        (lambda: hop(kp=inf), b'nele_drift_hop', b'kp'),
        (lambda: hop(kp=nan), b'nele_drift_hop', b'kp'),
        (lambda: hop(ki=-1.0), b'nele_drift_hop', b'ki'),
        (lambda: hop(ki=inf), b'nele_drift_hop', b'ki'),
        (lambda: hop(ki=nan), b'nele_drift_hop', b'ki'),
        (lambda: lib.nele_drift_init(None, LL(need), B, Q, None), b'nele_drift_init', b'state'),
        (lambda: lib.nele_drift_init(fake, LL(need - 1), B, Q, None), b'nele_drift_init', b'nele_drift_state_bytes'),
        (lambda: lib.nele_drift_init(fake, LL(need), 0, Q, None), b'nele_drift_init', b'max_streams'),
        (lambda: lib.nele_drift_init(fake, LL(need), B, 1, None), b'nele_drift_init', b'blocks'),
        (lambda: lib.nele_drift_init(odd, LL(need), B, Q, None), b'nele_drift_init', b'256-byte aligned'),
        (lambda: lib.nele_drift_reset(None, LL(need), B, Q, None, None), b'nele_drift_reset', b'state'),
        (lambda: lib.nele_drift_reset(fake, LL(need - 1), B, Q, None, None), b'nele_drift_reset', b'nele_drift_state_bytes'),
        (lambda: lib.nele_drift_reset(fake, LL(need), -3, Q, None, None), b'nele_drift_reset', b'max_streams'),
        (lambda: lib.nele_drift_reset(fake, LL(need), B, 65, None, None), b'nele_drift_reset', b'blocks'),
        (lambda: lib.nele_drift_reset(odd, LL(need), B, Q, None, None), b'nele_drift_reset', b'256-byte aligned'),
        (lambda: lib.nele_drift_set_rate(None, LL(need), B, Q, None, fake, None), b'nele_drift_set_rate', b'state'),
        (lambda: lib.nele_drift_set_rate(fake, LL(need - 1), B, Q, None, fake, None), b'nele_drift_set_rate', b'nele_drift_state_bytes'),
        (lambda: lib.nele_drift_set_rate(fake, LL(need), B, Q, None, None, None), b'nele_drift_set_rate', b'rate_dev'),
        (lambda: lib.nele_drift_set_rate(fake, LL(need), B, 65, None, fake, None), b'nele_drift_set_rate', b'blocks'),
        (lambda: lib.nele_drift_set_rate(odd, LL(need), B, Q, None, fake, None), b'nele_drift_set_rate', b'256-byte aligned'),
        (lambda: lib.nele_drift_status(None, LL(need), B, Q, fake, None), b'nele_drift_status', b'state'),
        (lambda: lib.nele_drift_status(fake, LL(need - 1), B, Q, fake, None), b'nele_drift_status', b'nele_drift_state_bytes'),
        (lambda: lib.nele_drift_status(fake, LL(need), B, Q, None, None), b'nele_drift_status', b'info'),
        (lambda: lib.nele_drift_status(fake, LL(need), B, 1, fake, None), b'nele_drift_status', b'blocks'),
        (lambda: lib.nele_drift_status(odd, LL(need), B, Q, fake, None), b'nele_drift_status', b'256-byte aligned'),
        (lambda: lib.nele_drift_taps(None, LL(need), B, Q, fake, None), b'nele_drift_taps', b'state'),
        (lambda: lib.nele_drift_taps(fake, LL(need - 1), B, Q, fake, None), b'nele_drift_taps', b'nele_drift_state_bytes'),
        (lambda: lib.nele_drift_taps(fake, LL(need), B, Q, None, None), b'nele_drift_taps', b'taps_out_dev'),
        (lambda: lib.nele_drift_taps(fake, LL(need), 0, Q, fake, None), b'nele_drift_taps', b'max_streams'),
        (lambda: lib.nele_drift_taps(odd, LL(need), B, Q, fake, None), b'nele_drift_taps', b'256-byte aligned'),
    ]
    for i, (fn, name, what) in enumerate(cases):
        assert fn() == -1, (i, name, what)
        msg = _err()
        assert name in msg and what in msg, (i, msg)


class _Stub:
    def __init__(self, S, Q=None):
        import torch
        self.S, self.Q, self.P, self.device, self.log = S, Q, 4, torch.device('cpu'), []

    # the search
    def delays(self):
        import torch
        self.log.append('delays')
        return torch.tensor([1, -1, 2][:self.S], dtype=torch.int32)

    # the canceller
    def reset_flagged(self, flags):
        self.log.append(('reset_flagged', flags.tolist()))

    def echo_path(self, slots=None):
        return ('path', slots)

    def reset(self, slots):
        self.log.append(('reset', list(slots)))


class _StubSearch(_Stub):
    def process(self, mic, played, active=None, out=None):
        self.log.append(('search', None if active is None else list(active)))
        return 5.0 * played


class _StubDrift(_Stub):
    def process(self, mic, played, base_hops, active=None, adapt=None, out=None, want_snapped=False):
        import torch
        self.log.append(('drift', base_hops.tolist(), None if active is None else list(active), adapt, want_snapped))
        return 2.0 * played, torch.tensor([0, 1, 0][:self.S], dtype=torch.uint8)


class _StubAec(_Stub):
    def process(self, mic, played, active=None, adapt=None, want_echo=False, out=None):
        self.log.append(('aec', None if active is None else list(active), adapt, want_echo, out))
        return (mic - played, 3.0 * played) if want_echo else mic - played


def test_python_classes_reject_bad_settings_before_touching_a_device():
    from nele_gan_amd.drift import DriftCompensator, DriftTrackedEchoCanceller
    nan = float('nan')
    for kw, what in (({'streams': 0}, 'streams'), ({'blocks': 1}, 'blocks'), ({'blocks': 65}, 'blocks'), ({'lam_fast': 0.0}, 'lam_fast'),
                     ({'lam_fast': nan}, 'lam_fast'), ({'lam_slow': 0.9}, 'lam_slow'), ({'lam_slow': 1.0}, 'lam_slow'), ({'kp': -1.0}, 'kp'),
                     ({'kp': nan}, 'kp'), ({'ki': -1.0}, 'ki'), ({'ki': float('inf')}, 'ki')):
        with pytest.raises(ValueError, match=what):
            DriftCompensator(**dict({'streams': 2}, **kw))
    with pytest.raises(ValueError, match='streams'):
        DriftTrackedEchoCanceller(_StubSearch(2, 8), _StubDrift(2, 8), _StubAec(3))
    with pytest.raises(ValueError, match='streams'):
        DriftTrackedEchoCanceller(_StubSearch(3, 8), _StubDrift(2, 8), _StubAec(2))
    with pytest.raises(ValueError, match='blocks'):
        DriftTrackedEchoCanceller(_StubSearch(2, 8), _StubDrift(2, 7), _StubAec(2))


def test_drift_tracked_canceller_bookkeeping_on_stubs():
    """process = the search; drift.process on the search's device delays; the canceller restarted where the mask says; aec.process
    on the compensator's output - in that order"""
    import torch
    from nele_gan_amd.drift import DriftTrackedEchoCanceller
    S, W = 3, 2 * HOP
    search, drift, aec = _StubSearch(S, 8), _StubDrift(S, 8), _StubAec(S)
    log = []
    search.log = drift.log = aec.log = log
    comp = DriftTrackedEchoCanceller(search, drift, aec)
    assert (comp.S, comp.P, comp.device) == (S, 4, aec.device)
    g = torch.Generator().manual_seed(5)
    mic, played = torch.rand(S, W, generator=g), torch.rand(S, W, generator=g)
    res, echo = comp.process(mic, played, active=[True, False, True], adapt=[True, True, False], want_echo=True, out=('res buffer', 'echo buffer'))
    assert log == [('search', [True, False, True]), 'delays', ('drift', [1, -1, 2], [True, False, True], None, True),
                   ('reset_flagged', [0, 1, 0]), ('aec', [True, False, True], [True, True, False], True, ('res buffer', 'echo buffer'))]
    assert torch.equal(res, mic - 2.0 * played) and torch.equal(echo, 6.0 * played)
    del log[:]
    assert torch.equal(comp.process(mic, played), mic - 2.0 * played) and log[-1] == ('aec', None, None, False, None)
    assert comp.echo_path([1]) == ('path', [1])
    del log[:]
    comp.reset([2, 0])
    assert log == [('reset', [2, 0])] * 3


# ---------------------------------------------------------------------------------------------------------------- the reference alone
def test_reference_table_is_the_formula_and_continuous_across_whole_samples():
    T = table()
    assert T.shape == (65, 64)
    for p, k in ((0, 31), (0, 0), (17, 40), (63, 63), (64, 32), (32, 31), (64, 0)):
        t = k - 31 - p / 64.0
        want = np.sinc(t) * np.i0(8.0 * np.sqrt(max(0.0, 1.0 - (t / 32.0) ** 2))) / np.i0(8.0)
        assert abs(T[p, k] - want) <= 1e-15, (p, k)
    assert T[0, 31] == 1.0 and not T[0, :31].any() and not T[0, 32:].any()            # row 0 is a pure delay of 31 samples
    assert np.array_equal(T[64, 1:], T[0, :-1]) and T[64, 0] == 0.0                   # row 64 is row 0 one tap later
    dc = np.abs(T.sum(axis=1) - 1.0).max()
    print('largest |DC gain - 1| over the 65 rows: %.3g' % dc)
    assert dc <= 4 * 2.2e-5


def _sinusoid_deviation(freq, rate, hops=24, Q=4, base=1):
    n = hops * HOP
    w = 2.0 * np.pi * freq / 16000.0
    x = np.sin(w * np.arange(n)).astype(np.float32)
    r = DriftRef(Q, kp=0.0, ki=0.0)
    r.set_rate(rate)
    r.begin_call(base)
    out, taus = [], []
    for k in range(hops):
        taus.append(r.tau + rate * (np.arange(HOP) + 1.0))
        out.append(r.hop(np.zeros(HOP), x[k * HOP:(k + 1) * HOP]))
    assert r.rate == rate and abs(r.tau - (HOP * base + n * rate)) < 1e-9
    want = np.sin(w * (np.arange(n) - np.concatenate(taus)))
    return np.abs(np.concatenate(out) - want)[3 * HOP:].max(), r


@pytest.mark.parametrize('freq,measured', [(1000.0, 2.5e-5), (7000.0, 2.3e-4)])
def test_reference_warp_delays_a_sinusoid_by_tau(freq, measured):
    """fixed rate, kp = ki = 0: a unit sinusoid comes out delayed by tau(n), tau crossing whole samples and every table row; the bound is
    four times the deviation DESIGN.md section 19 gives (the reference's own: 2.63e-5 at 1 kHz, 2.32e-4 at 7 kHz; float32 output)"""
    for rate in (5e-4, -5e-4, MAX_RATE):
        dev, r = _sinusoid_deviation(freq, rate)
        print('%g Hz, rate %g: largest deviation %.3g' % (freq, rate, dev))
        assert dev <= 4 * measured
        assert abs(r.tau - HOP) > 2.0                                                 # more than 128 rows and two whole samples


def test_reference_reads_stay_inside_the_ring_at_the_limits():
    Q = 4
    for tau, rate in ((TAU_MIN, -MAX_RATE), (TAU_MIN, MAX_RATE), (tau_max(Q), MAX_RATE), (tau_max(Q), -MAX_RATE)):
        r = DriftRef(Q, kp=0.0, ki=0.0)
        r.begin_call(0)
        r.tau = tau
        r.set_rate(rate)
        x = np.random.default_rng(3).standard_normal(12 * HOP).astype(np.float32)
        r.run(np.zeros(12 * HOP), x, 0)
        assert 0 <= r.lowest_read and r.highest_read <= r.R * HOP - 1, (tau, rate, r.lowest_read, r.highest_read)
        assert TAU_MIN <= r.tau <= tau_max(Q)
    assert tau_max(Q) == 256 * 7 - 33 and TAU_MIN == 31.0


HOPS, BULK, BASE, Q, P = 1200, 2000, 7, 8, 4
_LOOPS = {}


def _loop(ppm, enr_db=10.0, free=False, silent=False):
    """the reference chain over 1200 hops: DriftRef (snapped to the known base) ahead of AecRef (P = 4), and AecRef on `played` delayed by
    the whole hops alone -> dict (computed once, shared, never changed)"""
    key = (ppm, enr_db, free, silent)
    if key not in _LOOPS:
        s = DC.echo_free(HOPS) if free else DC.scenario(ppm, enr_db, 1, HOPS, bulk=BULK, silent=silent)
        r, aec = DriftRef(Q), AecRef(P)
        r.begin_call(BASE)
        y, est, taus = [], [], []
        for k in range(HOPS):
            d = s['mic'][k * HOP:(k + 1) * HOP]
            y.append(aec.hop(d, r.hop(d, s['played'][k * HOP:(k + 1) * HOP]))[1])
            est.append(r.drift_ppm)
            taus.append(r.tau)
        out = {'s': s, 'ref': r, 'y': np.concatenate(y), 'ppm': np.array(est), 'tau': np.array(taus)}
        if not free and not silent:
            whole = np.concatenate([np.zeros(BASE * HOP, np.float32), s['played']])[:HOPS * HOP]
            out['y_plain'] = AecRef(P).run(s['mic'], whole)[1]
        _LOOPS[key] = out
    return _LOOPS[key]


def test_reference_closed_loop_at_100_ppm_recovers_the_echo_reduction():
    """ENR 10 dB, path 700 taps / 0.08 s behind 2000 samples.  This reference: 13.43 dB against 7.72 dB over hops 900 .. 1199, the
    estimate 100.13 ppm at hop 1199"""
    c = _loop(100.0)
    comp, plain = (DC.window_db(c['s']['echo'], c[k], 900, 1200) for k in ('y', 'y_plain'))
    print('+100 ppm: %.2f dB compensated, %.2f dB on the whole-hop delay alone; estimate %.2f ppm' % (comp, plain, c['ppm'][-1]))
    assert comp >= 11.0 and comp >= plain + 3.0
    assert abs(c['ppm'][-1] - 100.0) <= 5.0


def test_reference_closed_loop_at_0_ppm_costs_nothing():
    """this reference: 12.06 dB against 12.08 dB, the estimate 1.27 ppm at hop 1199"""
    c = _loop(0.0)
    comp, plain = (DC.window_db(c['s']['echo'], c[k], 900, 1200) for k in ('y', 'y_plain'))
    print('0 ppm: %.2f dB compensated, %.2f dB without; estimate %.2f ppm' % (comp, plain, c['ppm'][-1]))
    assert abs(comp - plain) <= 0.1
    assert abs(c['ppm'][-1]) <= 3.0


def test_reference_wanders_little_on_an_echo_free_microphone():
    """toy noise only against the speech far end.  This reference: 3.36 ppm, tau within 0.40 samples of the base"""
    c = _loop(0.0, free=True)
    print('echo-free: largest |estimate| %.2f ppm, largest |tau - base| %.2f samples' % (np.abs(c['ppm']).max(), np.abs(c['tau'] - BASE * HOP).max()))
    assert np.abs(c['ppm']).max() <= 20.0


def test_reference_holds_still_while_the_far_end_is_silent():
    c = _loop(0.0, silent=True)
    assert c['ref'].n == HOPS                                                         # the loop was closed: it had nothing to move on
    assert np.array_equal(c['ppm'], np.zeros(HOPS)) and np.array_equal(c['tau'], np.full(HOPS, float(BASE * HOP)))
    assert c['ref'].rate.hex() == (0.0).hex()


def test_reference_snap_keeps_the_rate_and_clears_the_estimator():
    s = DC.scenario(100.0, 10.0, 1, 80, bulk=BULK)
    r = DriftRef(Q)
    assert r.begin_call(-1) is False and r.begin_call(Q) is False and r.base == -1
    assert not r.run(s['mic'][:4 * HOP], s['played'][:4 * HOP], -1).any() and (r.n, r.tau, r.snaps) == (0, 0.0, 0)
    assert np.array_equal(r.hist[-4 * HOP:], s['played'][:4 * HOP].astype(np.float64))     # unlocked: the ring still fills
    r.run(s['mic'][4 * HOP:60 * HOP], s['played'][4 * HOP:60 * HOP], BASE)
    assert (r.base, r.snaps, r.n) == (BASE, 1, 56) and r.rate != 0.0 and r.C_s.any()
    rate, hist = r.rate, r.hist.copy()
    assert r.begin_call(BASE) is False and r.begin_call(-1) is False and r.begin_call(64) is False and r.n == 56
    assert r.begin_call(3) is True
    assert (r.tau, r.base, r.snaps, r.n, r.delta) == (768.0, 3, 2, 0, 0.0) and r.rate.hex() == rate.hex()
    assert not r.u_prev.any() and not r.S_d.any() and not r.S_u.any() and not r.C_f.any() and not r.C_s.any()
    assert np.array_equal(r.hist, hist)
    assert r.begin_call(0) is True and r.tau == TAU_MIN                               # a base of 0: 31 samples ahead of the main tap at the least
    r.set_rate(2 * MAX_RATE)
    assert r.rate.hex() == rate.hex()                                                 # out of range: unchanged


def test_reference_perturbation_figure():
    """tau and C_s moved by 1e-15 relative after every hop, the GPU test's closed-loop scenarios (264 hops at +500 ppm): how far tau and
    rate end from the unperturbed run.  The largest is DC.PERTURBED_TAU, the figure of DESIGN.md section 19 that bounds the kernel"""
    worst_tau = worst_rate = 0.0
    for q, rows in DC.GPU_LOOPS.items():
        for slot in range(len(rows)):
            s = DC.gpu_loop(q, slot)
            a, b = DriftRef(q), DriftRef(q)
            a.begin_call(rows[slot][0])
            b.begin_call(rows[slot][0])
            for k in range(DC.GPU_HOPS):
                d, x = s['mic'][k * HOP:(k + 1) * HOP], s['played'][k * HOP:(k + 1) * HOP]
                a.hop(d, x)
                b.hop(d, x)
                b.tau, b.C_s = b.tau * (1.0 + 1e-15), b.C_s * (1.0 + 1e-15)
                worst_tau, worst_rate = max(worst_tau, abs(a.tau - b.tau)), max(worst_rate, abs(a.rate - b.rate))
    print('perturbed by 1e-15 per hop: tau moved by at most %.3g samples, rate by %.3g' % (worst_tau, worst_rate))
    assert 0.1 * DC.PERTURBED_TAU <= worst_tau <= DC.PERTURBED_TAU
    assert 0.1 * DC.PERTURBED_RATE <= worst_rate <= DC.PERTURBED_RATE
    assert 100.0 * DC.PERTURBED_TAU <= 1e-6                                           # the cap of the GPU bound does not bite
