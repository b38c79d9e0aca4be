"""CPU: the active-speech-level contract.  tests/p56_ref.py (the windowed restatement the kernel follows) against vectors generated from
the reference's asl_P56 (tests/golden/p56.npz, make_golden_p56.py): activity counters exactly, sum of squares to 1e-11 relative (n eps for
n <= 128 000 float64 additions), the result triple to 1e-9 relative (the same bisection path: every golden input keeps every comparison
of the 0.5 dB bisection at least 1e-6 dB from flipping, recorded in the file).  Plus the constants the kernel source carries and the
exported symbols."""
import ctypes
import os
import re

import numpy as np
import pytest

import p56_cases
import p56_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def golden():
    return p56_cases.load()


def test_golden_set_is_what_the_issue_asks_for(golden):
    g, cases = golden
    names = [n for n, _ in cases]
    assert 'toy_train' in names and 'toy_test' in names
    assert 'pauses' in names and int(g['status'][names.index('pauses')]) == 0          # the hangover boundary on exact sample distances
    assert {63871, 128000} <= set(int(v) for v in g['n'])
    assert sorted(int(s) for s in g['status'] if s) == [p56_ref.SILENT, p56_ref.BELOW_MARGIN, p56_ref.NO_CROSSING]
    ok = g['status'] == 0
    assert (g['margin_db'][ok] >= 1e-6).all() and (g['delta_margin_db'][ok] >= 1e-6).all()
    # the scaled versions move the crossing to other thresholds than the level-0.03 inputs'
    cross = [int(np.argmax(g['counts'][i] == 1)) for i in range(len(names)) if ok[i]]
    assert len(set(cross)) >= 3
    # the reference's figures for the two toy files
    for name, asl, act in (('toy_train', 9.1893e-4, 0.9794), ('toy_test', 9.2860e-4, 0.9692)):
        i = names.index(name)
        assert abs(g['asl_msq'][i] - asl) < 1e-8 and abs(g['actfact'][i] - act) < 1e-4


def test_restatement_equals_the_reference_vectors(golden):
    g, cases = golden
    for i, (name, x) in enumerate(cases):
        r = p56_ref.level(x)
        assert (r['counts'] == g['counts'][i]).all(), (name, r['counts'].tolist(), g['counts'][i].tolist())
        assert r['status'] == int(g['status'][i]), name
        if float(g['sq'][i]) > 0:
            assert p56_cases.rel(r['sq'], g['sq'][i]) <= 1e-11, name
        else:
            assert r['sq'] == 0.0
        for k in ('asl_msq', 'actfact', 'c0'):
            if r['status'] == 0:
                assert p56_cases.rel(r[k], g[k][i]) <= 1e-9, (name, k, r[k], float(g[k][i]))
            else:
                assert r[k] == 0.0 and float(g[k][i]) == 0.0


def test_windowed_counts_equal_the_hangover_loop_on_a_gappy_envelope():
    """the windowed form against a direct per-sample hangover state machine, on an envelope with gaps around the hangover length"""
    rs = np.random.RandomState(5)
    q = np.zeros(30000)
    for start, width, amp in ((100, 50, 0.3), (3400, 10, 2e-3), (6601, 1, 0.6), (9802, 1, 0.6), (13004, 1, 0.6), (20000, 4000, 1e-4), (29990, 10, 0.01)):
        q[start:start + width] = amp * (0.5 + 0.5 * rs.rand(width))
    got = p56_ref.activity_counts(q)
    want = np.zeros(p56_ref.NTHR, dtype=np.int64)
    for j, c in enumerate(p56_ref.THRESHOLDS):
        hang, n = p56_ref.HANG, 0
        for v in q:
            if v >= c:
                n, hang = n + 1, 0
            elif hang < p56_ref.HANG:
                n, hang = n + 1, hang + 1
        want[j] = n + 1
    assert (got == want).all(), (got.tolist(), want.tolist())


def test_kernel_source_carries_the_reference_constants():
    src = open(os.path.join(ROOT, 'nele_gan_amd', 'csrc', 'level.hip')).read()
    g_hex = re.search(r'#define P56_G (\S+)', src).group(1)
    assert float.fromhex(g_hex) == float(np.exp(-1 / (16000 * 0.03)))
    assert float(re.search(r'#define P56_EPS (\S+)', src).group(1)) == float(np.finfo(float).eps)
    assert int(re.search(r'#define P56_HANG (\d+)', src).group(1)) == int(np.ceil(16000 * 0.2))
    assert float(re.search(r'#define P56_MARGIN (\S+)', src).group(1)) == 15.9
    mk = open(os.path.join(ROOT, 'nele_gan_amd', 'csrc', 'Makefile')).read()
    assert 'level' in re.search(r'^EXACT := (.*)$', mk, flags=re.M).group(1).split()      # built without FMA contraction


def test_library_exports_the_level_and_mixing_symbols():
    hdr = open(os.path.join(ROOT, 'include', 'nele_hip.h')).read()
    for name in ('libnele_hip.so', 'libnele_hip_ab.so'):
        lib = ctypes.CDLL(os.path.join(ROOT, 'nele_gan_amd', name))
        for sym in ('nele_asl_p56_var', 'nele_asl_p56_workspace_bytes', 'nele_mix_noise_var'):
            assert sym in hdr and hasattr(lib, sym), (name, sym)
    lib.nele_asl_p56_workspace_bytes.restype = ctypes.c_longlong
    assert lib.nele_asl_p56_workspace_bytes(256, 64000) >= 0
    for flag in ('NELE_P56_SILENT', 'NELE_P56_BELOW_MARGIN', 'NELE_P56_NO_CROSSING', 'NELE_MIX_ZERO_NOISE', 'NELE_MIX_ZERO_LEVEL'):
        assert re.search(r'#define %s \d+' % flag, hdr), flag


def test_python_binding_declares_the_new_entry_points_and_rejects_bad_arguments_without_a_gpu():
    from nele_gan_amd import _lib, asl_P56
    for sym in ('nele_asl_p56_var', 'nele_asl_p56_workspace_bytes', 'nele_mix_noise_var'):
        assert sym in _lib._SIGS
    assert _lib.lib.nele_asl_p56_var(None, None, 0, 0, None, 0, None, None, None, None, None, None, None) == -1
    assert b'nele_asl_p56_var' in _lib.lib.nele_last_error_string()
    assert _lib.lib.nele_mix_noise_var(None, None, 0, 0, None, None, None, None, None, 0, 0, None, None, None, None) == -1
    assert (asl_P56.SILENT, asl_P56.BELOW_MARGIN, asl_P56.NO_CROSSING) == (p56_ref.SILENT, p56_ref.BELOW_MARGIN, p56_ref.NO_CROSSING)
    x = np.zeros(100, dtype=np.float32)
    with pytest.raises(ValueError, match='16000'):
        asl_P56.asl_P56(x, 8000, 16)
    with pytest.raises(ValueError, match='nbits'):
        asl_P56.asl_P56(x, 16000, 12)
