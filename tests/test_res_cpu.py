"""CPU: the residual-echo suppressor's C ABI (nele_res_* of include/nele_hip_ext.h: exported by both libraries, state-size arithmetic,
bad arguments rejected without a GPU; the header and the binding as a whole: tests/test_abi_ext_cpu.py), the numpy reference tests/res_ref.py on its own
against DESIGN.md section 17's pass-through and suppression figures, and SuppressedEchoCanceller's bookkeeping on stubs."""
import ctypes
import os

import numpy as np
import pytest

import aec_cases as C
from res_cases import SCENARIOS, figures, ref_run
from res_ref import HOP, NBINS, ResRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LL = ctypes.c_longlong
ENTRY_POINTS = ('nele_res_state_bytes', 'nele_res_stream_record_bytes', 'nele_res_init', 'nele_res_reset', 'nele_res_hop')


def _lib():
    from nele_gan_amd import _lib
    return _lib.lib


def _err():
    return _lib().nele_last_error_string()


# ------------------------------------------------------------------------------------------------------------------------ the C ABI
def test_both_libraries_export_the_entry_points():
    for name in ('libnele_hip.so', 'libnele_hip_ab.so'):
        lib = ctypes.CDLL(os.path.join(ROOT, 'nele_gan_amd', name))
        assert [s for s in ENTRY_POINTS if not hasattr(lib, s)] == [], name


def test_state_bytes_are_a_header_plus_one_record_per_stream():
    lib = _lib()
    rec = lib.nele_res_stream_record_bytes()
    # e_prev, y_prev (float32), ola, S_ee, S_yy (float64), S_ey (complex)
    assert rec >= 2 * 256 * 4 + 256 * 8 + 2 * 257 * 8 + 257 * 16 and rec % 256 == 0 and rec < 16384
    header = lib.nele_res_state_bytes(1) - rec
    assert 0 < header <= 4096
    for B in (1, 2, 16, 1024, 4096, 1 << 20):
        assert lib.nele_res_state_bytes(B) == header + B * rec
    for B in (0, -1, (1 << 20) + 1):
        assert lib.nele_res_state_bytes(B) == -1


def test_bad_arguments_are_rejected_without_a_gpu():
    lib = _lib()
    B = 4
    need = lib.nele_res_state_bytes(B)
    fake = ctypes.c_void_p(1 << 20)                                 # never dereferenced: every call below fails its checks first
    odd = ctypes.c_void_p((1 << 20) + 16)
    nan, inf = float('nan'), float('inf')

    def hop(state=fake, nbytes=need, S=B, residual=fake, echo=fake, nh=1, beta=2.0, gmin=0.1, out=fake):
        return lib.nele_res_hop(state, LL(nbytes), S, residual, echo, None, nh, beta, gmin, out, None, None)

    cases = [
        (lambda: hop(state=None), b'nele_res_hop', b'state'),
        (lambda: hop(nbytes=need - 1), b'nele_res_hop', b'nele_res_state_bytes'),
        (lambda: hop(S=0), b'nele_res_hop', b'max_streams'),
        (lambda: hop(S=(1 << 20) + 1, nbytes=1 << 40), b'nele_res_hop', b'max_streams'),
        (lambda: hop(state=odd), b'nele_res_hop', b'256-byte aligned'),
        (lambda: hop(residual=None), b'nele_res_hop', b'residual'),
        (lambda: hop(echo=None), b'nele_res_hop', b'echo'),
        (lambda: hop(out=None), b'nele_res_hop', b'out'),
        (lambda: hop(nh=0), b'nele_res_hop', b'nh'),
        (lambda: hop(nh=(1 << 20) + 1), b'nele_res_hop', b'nh'),
        (lambda: hop(beta=-0.5), b'nele_res_hop', b'beta'),
        (lambda: hop(beta=nan), b'nele_res_hop', b'beta'),
        (lambda: hop(beta=inf), b'nele_res_hop', b'beta'),
        (lambda: hop(gmin=0.0), b'nele_res_hop', b'gmin'),
        (lambda: hop(gmin=1.5), b'nele_res_hop', b'gmin'),
        (lambda: hop(gmin=nan), b'nele_res_hop', b'gmin'),
        (lambda: lib.nele_res_init(None, LL(need), B, None), b'nele_res_init', b'state'),
        (lambda: lib.nele_res_init(fake, LL(need - 1), B, None), b'nele_res_init', b'nele_res_state_bytes'),
        (lambda: lib.nele_res_init(fake, LL(need), 0, None), b'nele_res_init', b'max_streams'),
        (lambda: lib.nele_res_init(odd, LL(need), B, None), b'nele_res_init', b'256-byte aligned'),
        (lambda: lib.nele_res_reset(None, LL(need), B, None, None), b'nele_res_reset', b'state'),
        (lambda: lib.nele_res_reset(fake, LL(need - 1), B, None, None), b'nele_res_reset', b'nele_res_state_bytes'),
        (lambda: lib.nele_res_reset(fake, LL(need), -3, None, None), b'nele_res_reset', b'max_streams'),
        (lambda: lib.nele_res_reset(odd, LL(need), B, None, None), b'nele_res_reset', b'256-byte aligned'),
    ]
    for i, (fn, name, what) in enumerate(cases):
        assert fn() == -1, (i, name, what)
        msg = _err()
        assert name in msg and what in msg, (i, msg)


def test_python_class_rejects_bad_settings_before_touching_a_device():
    from nele_gan_amd.res import ResidualEchoSuppressor
    for kw, what in (({'streams': 0}, 'streams'), ({'beta': -1.0}, 'beta'), ({'beta': float('nan')}, 'beta'), ({'gmin': 0.0}, 'gmin'),
                     ({'gmin': 1.01}, 'gmin'), ({'gmin': float('nan')}, 'gmin')):
        with pytest.raises(ValueError, match=what):
            ResidualEchoSuppressor(**dict({'streams': 2}, **kw))


# ---------------------------------------------------------------------------------------------------------------- the reference alone
def test_reference_without_an_echo_estimate_is_a_delay_of_one_hop():
    """echo = 0 throughout: S_ey and R stay zero, G is exactly 1 and sqrt-Hann analysis and synthesis overlap-add to the input, one hop
    late, within 1e-14 max |e| (the prototype gave 4e-17; exact zeros come back as about 1e-17, so this is not a bitwise check)"""
    e = C.scenario(1, 700, 0.08, 10.0, hops=40)['mic']
    out, G = ResRef().run(e, np.zeros_like(e))
    assert np.array_equal(G, np.ones((40, NBINS)))
    assert out.dtype == np.float32 and np.abs(out[:HOP]).max() <= 1e-14 * np.abs(e).max()      # hop 0: the zero history, to rounding
    worst = float(np.abs(out[HOP:].astype(np.float64) - e[:-HOP]).max() / np.abs(e).max())
    print('echo = 0: largest |out - input one hop earlier| = %.3g max |e| (bound 1e-14)' % worst)
    assert worst <= 1e-14


@pytest.mark.parametrize('seed,taps,t60,enr_db,P', SCENARIOS)
def test_reference_suppresses_the_residual_echo_and_keeps_the_noise(seed, taps, t60, enr_db, P):
    """DESIGN.md section 17's table: at least 3 dB off the residual echo over the second half (the prototype: 4.60, 4.51, 5.77 dB),
    the noise level changed by at most 1.5 dB (-1.27, -1.01, -1.37 dB); echo part + noise part = output to float32 rounding (three
    roundings of values no larger than the output's peak: 3 * 2^-24 of it)"""
    run = ref_run(seed, taps, t60, enr_db, P)
    sup, lvl, split = figures(run['e'], run['noise'], run['out'], run['G'])
    print('seed %d taps %d T60 %g ENR %g P %d: residual echo suppressed %.2f dB, noise level %+.2f dB, split %.3g' % (seed, taps, t60, enr_db, P, sup, lvl, split))
    assert run['G'].shape == (264, NBINS) and run['G'].min() >= 0.1 and run['G'].max() <= 1.0
    assert sup >= 3.0
    assert abs(lvl) <= 1.5
    assert split <= 3.0 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ SuppressedEchoCanceller's bookkeeping
class _StubAec:
    def __init__(self, S):
        import torch
        self.S, self.P, self.device, self.calls, self.resets = S, 4, torch.device('cpu'), [], []

    def process(self, mic, played, active=None, adapt=None, want_echo=False, out=None):
        self.calls.append((mic.clone(), played.clone(), None if active is None else np.array(active, dtype=bool), adapt, want_echo, out))
        return (mic - played, 3.0 * played) if want_echo else mic - played

    def echo_path(self, slots=None):
        return ('path', slots)

    def reset(self, slots):
        self.resets.append(list(slots))


class _StubRes:
    def __init__(self, S):
        self.S, self.calls, self.resets, self.hops = S, [], [], np.zeros(S, dtype=np.int64)

    def process(self, residual, echo, active=None, want_gains=False, out=None):
        self.calls.append((residual.clone(), echo.clone(), None if active is None else np.array(active, dtype=bool), want_gains, out))
        self.hops[slice(None) if active is None else np.array(active, dtype=bool)] += residual.shape[1] // HOP
        return residual - 0.25 * echo

    def reset(self, slots):
        self.resets.append(list(slots))
        self.hops[list(slots)] = 0


class _StubRt:
    def __init__(self, S):
        self.S, self.n, self.resets = S, 0, []

    def process(self, clean, noise, active=None):
        self.n += 1
        return clean + 0.5 * noise + float(self.n)

    def finish(self, slots, clean_tail, noise_tail, tail_lengths):
        return noise_tail

    def reset(self, slots):
        self.resets.append(list(slots))


def test_suppressed_canceller_bookkeeping_on_stubs():
    import torch
    from nele_gan_amd.aec import EchoCancellingEnhancer
    from nele_gan_amd.res import SuppressedEchoCanceller
    S, W = 3, 2 * HOP
    aec, res = _StubAec(S), _StubRes(S)
    sup = SuppressedEchoCanceller(aec, res)
    assert (sup.S, sup.P, sup.device) == (S, 4, aec.device)
    g = torch.Generator().manual_seed(5)
    mic, played = torch.rand(S, W, generator=g), torch.rand(S, W, generator=g)
    # process = res.process(*aec.process(mic, played, ..., want_echo=True), active): the canceller is always asked for its echo
    o, echo = sup.process(mic, played, active=[True, False, True], adapt=[True, True, False], want_echo=True, out=('res buffer', 'echo buffer'))
    m, p, act, adapt, want_echo, out = aec.calls[0]
    assert torch.equal(m, mic) and torch.equal(p, played) and list(act) == [True, False, True] and adapt == [True, True, False]
    assert want_echo is True and out == (None, 'echo buffer')
    e, y, act, want_gains, out = res.calls[0]
    assert torch.equal(e, mic - played) and torch.equal(y, 3.0 * played) and list(act) == [True, False, True]
    assert want_gains is False and out == 'res buffer'
    assert torch.equal(echo, 3.0 * played)
    # a slot's first hop is the canceller's own residual of that hop (the suppressor's is its zero history); inactive slots are left alone
    want = (mic - played) - 0.75 * played
    first = want.clone()
    first[0, :HOP], first[2, :HOP] = (mic - played)[0, :HOP], (mic - played)[2, :HOP]
    assert torch.equal(o, first) and not torch.equal(o[0], want[0]) and torch.equal(o[1], want[1])
    second = want.clone()
    second[1, :HOP] = (mic - played)[1, :HOP]                                    # slot 1's first call is this one
    only = sup.process(mic, played)
    assert torch.equal(only, second) and aec.calls[1][2:] == (None, None, True, None) and res.calls[1][2:] == (None, False, None)
    assert torch.equal(sup.process(mic, played), want)                           # no slot is new any more
    assert sup.process(mic, played, out='res buffer') is not None and aec.calls[3][5] is None and res.calls[3][4] == 'res buffer'
    assert sup.echo_path([1]) == ('path', [1])
    sup.reset([2, 0])
    assert aec.resets == [[2, 0]] and res.resets == [[2, 0]]
    again = sup.process(mic, played)                                             # after a reset a slot is new again
    assert torch.equal(again[0, :HOP], (mic - played)[0, :HOP]) and torch.equal(again[1], want[1]) and torch.equal(again[:, HOP:], want[:, HOP:])
    with pytest.raises(ValueError, match='streams'):
        SuppressedEchoCanceller(_StubAec(2), _StubRes(3))
    # inside the closed loop: the enhancer is given the suppressed residual, the loop's own bookkeeping is unchanged
    aec, res, rt = _StubAec(S), _StubRes(S), _StubRt(S)
    loop = EchoCancellingEnhancer(rt, SuppressedEchoCanceller(aec, res))
    clean = [torch.rand(S, W, generator=g) for _ in range(3)]
    mics = [torch.rand(S, W, generator=g) for _ in range(3)]
    out0 = loop.process(clean[0], mics[0])
    assert torch.equal(aec.calls[0][1], torch.zeros(S, W)) and torch.equal(out0, clean[0] + 0.5 * mics[0] + 1.0)      # played = 0: residual = mic
    out1 = loop.process(clean[1], mics[1], active=[True, False, True])
    assert torch.equal(aec.calls[1][1], out0) and list(aec.calls[1][2]) == [True, False, True] and list(res.calls[1][2]) == [True, False, True]
    assert torch.equal(out1, clean[1] + 0.5 * ((mics[1] - out0) - 0.75 * out0) + 2.0)
    loop.process(clean[2], mics[2])
    assert torch.equal(aec.calls[2][1][1], out0[1]) and torch.equal(aec.calls[2][1][0], out1[0])
    loop.reset([1])
    assert rt.resets == [[1]] and aec.resets == [[1]] and res.resets == [[1]] and not loop.played[1].any()
    last = loop.finish([2], torch.rand(1, 100, generator=g), torch.rand(1, 100, generator=g), [100])
    assert last.shape == (1, HOP) and list(aec.calls[-1][2]) == [False, False, True] and list(res.calls[-1][2]) == [False, False, True]
    with pytest.raises(ValueError, match='streams'):
        EchoCancellingEnhancer(_StubRt(2), SuppressedEchoCanceller(_StubAec(3), _StubRes(3)))
