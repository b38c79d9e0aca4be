"""CPU: the echo canceller's C ABI (nele_aec_*: declared, exported, state-size arithmetic, bad arguments rejected without a GPU), the
numpy reference tests/aec_ref.py checked on its own against DESIGN.md section 14's properties, and the played / active bookkeeping of
nele_gan_amd.aec.EchoCancellingEnhancer on stub objects."""
import ctypes
import os
import re

import numpy as np
import pytest

import aec_cases as C
from aec_ref import HOP, AecRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LL = ctypes.c_longlong
ENTRY_POINTS = ('nele_aec_state_bytes', 'nele_aec_stream_record_bytes', 'nele_aec_init', 'nele_aec_reset', 'nele_aec_hop', 'nele_aec_echo_path')


def _lib():
    from nele_gan_amd import _lib, aec  # noqa: F401  (aec declares the signatures)
    return _lib.lib


def _err():
    return _lib().nele_last_error_string()


def test_header_declares_the_six_entry_points():
    src = open(os.path.join(ROOT, 'include', 'nele_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(nele_[a-z0-9_]+)\s*\(', src))
    assert set(ENTRY_POINTS) <= declared, sorted(set(ENTRY_POINTS) - declared)
    assert re.search(r'#define\s+NELE_AEC_SMOOTH\s+0\.9\b', src)


def test_library_exports_the_six_entry_points():
    lib = ctypes.CDLL(os.path.join(ROOT, 'nele_gan_amd', 'libnele_hip.so'))
    assert [s for s in ENTRY_POINTS if not hasattr(lib, s)] == []


def test_state_bytes_are_a_header_plus_one_record_per_stream():
    lib = _lib()
    for P in (1, 2, 3, 8, 31, 32):
        rec = lib.nele_aec_stream_record_bytes(P)
        assert rec >= (2 * P + 1) * 257 * 16 - 257 * 8 and rec % 256 == 0       # X ring, W (complex) and S_e (real), bins 0 and 256 real
        header = lib.nele_aec_state_bytes(1, P) - rec
        assert 0 < header <= 4096
        for B in (1, 2, 16, 1024, 4096):
            assert lib.nele_aec_state_bytes(B, P) == header + B * rec
    for B, P in ((0, 8), (-1, 8), (4, 0), (4, 33), (4, -2)):
        assert lib.nele_aec_state_bytes(B, P) == -1
    assert lib.nele_aec_stream_record_bytes(0) == -1 and lib.nele_aec_stream_record_bytes(33) == -1


def test_bad_arguments_are_rejected_without_a_gpu():
    lib = _lib()
    B, P = 4, 8
    need = lib.nele_aec_state_bytes(B, P)
    fake = ctypes.c_void_p(1 << 20)                                 # never dereferenced: every call below fails its checks first

    def hop(state=fake, nbytes=need, S=B, parts=P, mic=fake, played=fake, nh=1, mu=0.5, gamma=4.0, delta=1e-2, residual=fake):
        return lib.nele_aec_hop(state, LL(nbytes), S, parts, mic, played, None, None, nh, mu, gamma, delta, residual, None, None)

    cases = [
        (lambda: hop(parts=0, nbytes=1 << 40), b'nele_aec_hop', b'partitions'),
        (lambda: hop(parts=33, nbytes=1 << 40), b'nele_aec_hop', b'partitions'),
        (lambda: hop(nh=0), b'nele_aec_hop', b'nh'),
        (lambda: hop(mic=None), b'nele_aec_hop', b'mic'),
        (lambda: hop(played=None), b'nele_aec_hop', b'played'),
        (lambda: hop(residual=None), b'nele_aec_hop', b'residual'),
        (lambda: hop(state=None), b'nele_aec_hop', b'state'),
        (lambda: hop(nbytes=need - 1), b'nele_aec_hop', b'nele_aec_state_bytes'),
        (lambda: hop(S=0), b'nele_aec_hop', b'max_streams'),
        (lambda: hop(mu=0.0), b'nele_aec_hop', b'mu'),
        (lambda: hop(mu=2.0), b'nele_aec_hop', b'mu'),
        (lambda: hop(mu=float('nan')), b'nele_aec_hop', b'mu'),
        (lambda: hop(gamma=-1e-9), b'nele_aec_hop', b'gamma'),
        (lambda: hop(delta=0.0), b'nele_aec_hop', b'delta'),
        (lambda: hop(state=ctypes.c_void_p((1 << 20) + 16)), b'nele_aec_hop', b'aligned'),
        (lambda: lib.nele_aec_init(None, LL(need), B, P, None), b'nele_aec_init', b'state'),
        (lambda: lib.nele_aec_init(fake, LL(need - 1), B, P, None), b'nele_aec_init', b'nele_aec_state_bytes'),
        (lambda: lib.nele_aec_init(fake, LL(1 << 40), B, 0, None), b'nele_aec_init', b'partitions'),
        (lambda: lib.nele_aec_init(fake, LL(1 << 40), B, 33, None), b'nele_aec_init', b'partitions'),
        (lambda: lib.nele_aec_reset(None, LL(need), B, P, None, None), b'nele_aec_reset', b'state'),
        (lambda: lib.nele_aec_reset(fake, LL(need - 1), B, P, None, None), b'nele_aec_reset', b'nele_aec_state_bytes'),
        (lambda: lib.nele_aec_echo_path(None, LL(need), B, P, fake, None), b'nele_aec_echo_path', b'state'),
        (lambda: lib.nele_aec_echo_path(fake, LL(need), B, P, None, None), b'nele_aec_echo_path', b'null h'),
        (lambda: lib.nele_aec_echo_path(fake, LL(need - 1), B, P, fake, None), b'nele_aec_echo_path', b'nele_aec_state_bytes'),
    ]
    for i, (fn, name, what) in enumerate(cases):
        assert fn() == -1, (i, name, what)
        msg = _err()
        assert name in msg and what in msg, (i, msg)


def test_python_classes_reject_bad_settings_before_touching_a_device():
    from nele_gan_amd.aec import EchoCanceller
    for kw, what in (({'streams': 0}, 'streams'), ({'partitions': 0}, 'partitions'), ({'partitions': 33}, 'partitions'), ({'mu': 0.0}, 'mu'),
                     ({'mu': 2.0}, 'mu'), ({'gamma': -1.0}, 'gamma'), ({'delta': 0.0}, 'delta')):
        with pytest.raises(ValueError, match=what):
            EchoCanceller(**dict({'streams': 2}, **kw))


# ---------------------------------------------------------------------------------------------------------------- the reference alone
def test_reference_output_is_the_convolution_with_its_own_echo_path():
    """y of a hop = (played history * echo_path() read before the hop) on that hop: overlap-save with constrained weights IS a linear
    convolution with the 256 P taps.  Bound 1e-12 (float64 transforms of 512 points on signals below 1)."""
    s = C.scenario(seed=5, taps=700, t60=0.08, enr_db=10.0, hops=40)
    ref = AecRef(3)
    worst = 0.0
    for m in range(40):
        h = ref.echo_path()
        _, y = ref.hop(s['mic'][m * HOP:(m + 1) * HOP], s['played'][m * HOP:(m + 1) * HOP])
        want = np.convolve(s['played'][:(m + 1) * HOP].astype(np.float64), h)[m * HOP:(m + 1) * HOP]
        worst = max(worst, float(np.abs(y - want).max()))
    assert 0.0 < np.abs(ref.echo_path()).max()
    assert worst <= 1e-12, worst


def test_reference_weights_stay_constrained():
    s = C.scenario(seed=6, taps=700, t60=0.08, enr_db=10.0, hops=60)
    ref = AecRef(3)
    ref.run(s['mic'], s['played'])
    g = np.fft.irfft(ref.W, 512, axis=1)
    assert np.abs(g[:, :HOP]).max() > 1e-2
    assert np.abs(g[:, HOP:]).max() < 1e-15


def test_reference_identifies_a_path_from_white_noise():
    """white far end, no near-end noise, 200 hops, P = 2, a 300-tap path: the estimate ends below -100 dB of the path's energy"""
    rng = np.random.default_rng(11)
    x = (0.1 * rng.standard_normal(200 * HOP)).astype(np.float32)
    h = C.echo_path(12, 300, 0.05)
    d = np.convolve(x.astype(np.float64), h)[:len(x)]
    ref = AecRef(2)
    ref.run(d, x)                                                    # the microphone in float64: no rounding floor under the estimate
    full = np.zeros(2 * HOP)
    full[:300] = h
    err_db = 10.0 * np.log10(np.sum((ref.echo_path() - full) ** 2) / np.sum(full ** 2))
    print('path error %.1f dB' % err_db)
    assert err_db < -100.0, err_db


# ------------------------------------------------------------------------------------------- EchoCancellingEnhancer's bookkeeping
class _StubAec:
    def __init__(self, S):
        import torch
        self.S, self.device, self.calls, self.resets = S, torch.device('cpu'), [], []

    def process(self, mic, played, active=None):
        self.calls.append((mic.clone(), played.clone(), None if active is None else np.array(active, dtype=bool)))
        return mic - played

    def reset(self, slots):
        self.resets.append(list(slots))


class _StubRt:
    def __init__(self, S):
        self.S, self.n, self.resets, self.finished = S, 0, [], []

    def process(self, clean, noise, active=None):
        self.n += 1
        return clean + 0.5 * noise + float(self.n)

    def finish(self, slots, clean_tail, noise_tail, tail_lengths):
        self.finished.append((list(slots), clean_tail.clone(), noise_tail.clone(), list(tail_lengths)))
        return noise_tail

    def reset(self, slots):
        self.resets.append(list(slots))


def test_closed_loop_bookkeeping_on_stubs():
    import torch
    from nele_gan_amd.aec import EchoCancellingEnhancer
    S, W = 3, 2 * HOP
    aec, rt = _StubAec(S), _StubRt(S)
    loop = EchoCancellingEnhancer(rt, aec)
    g = torch.Generator().manual_seed(3)
    clean = [torch.rand(S, W, generator=g) for _ in range(4)]
    mic = [torch.rand(S, W, generator=g) for _ in range(4)]
    out0 = loop.process(clean[0], mic[0])
    assert torch.equal(aec.calls[0][1], torch.zeros(S, W))                      # nothing played before the first call
    assert torch.equal(out0, clean[0] + 0.5 * mic[0] + 1.0)
    kept0 = out0.clone()
    out1 = loop.process(clean[1], mic[1])
    assert torch.equal(aec.calls[1][1], out0)                                    # what the last call returned is what was played
    assert torch.equal(out1, clean[1] + 0.5 * (mic[1] - out0) + 2.0)
    act = [True, False, True]
    out2 = loop.process(clean[2], mic[2], active=act)
    assert list(aec.calls[2][2]) == act
    out3 = loop.process(clean[3], mic[3])
    played = aec.calls[3][1]
    assert torch.equal(played[0], out2[0]) and torch.equal(played[2], out2[2])
    assert torch.equal(played[1], out1[1])                                       # the inactive slot keeps what it last played
    with pytest.raises(ValueError, match='hops per call'):
        loop.process(clean[0][:, :HOP], mic[0][:, :HOP])
    # reset: both objects, and the slot plays zeros again
    loop.reset([1])
    assert rt.resets == [[1]] and aec.resets == [[1]]
    before = loop.played.clone()
    assert not before[1].any() and before[0].any() and before[2].any()
    assert torch.equal(out0, kept0) and loop.played is not out3 and out3[1].any()     # what process() returned stays the caller's: reset changed the loop's copy
    # finish: tails padded to one hop, one canceller hop on those slots against the first hop of what they play
    ct, mt = torch.rand(2, 100, generator=g), torch.rand(2, 100, generator=g)
    last = loop.finish([2, 0], ct, mt, [100, 7])
    m, p, a = aec.calls[-1]
    assert m.shape == (S, HOP) and list(a) == [True, False, True]
    assert torch.equal(m[2, :100], mt[0]) and torch.equal(m[0, :100], mt[1]) and not m[:, 100:].any() and not m[1].any()
    assert torch.equal(p, before[:, :HOP])
    slots, c_tail, n_tail, r = rt.finished[0]
    assert slots == [2, 0] and r == [100, 7] and c_tail.shape == n_tail.shape == (2, HOP)
    assert torch.equal(c_tail[:, :100], ct) and not c_tail[:, 100:].any()
    assert torch.equal(n_tail, (m - p)[[2, 0]]) and torch.equal(last, n_tail)


def test_closed_loop_needs_matching_stream_counts():
    from nele_gan_amd.aec import EchoCancellingEnhancer
    with pytest.raises(ValueError, match='streams'):
        EchoCancellingEnhancer(_StubRt(2), _StubAec(3))
