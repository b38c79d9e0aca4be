"""CPU: the premises of the SIIB back-end stage tests (tests/test_siib_stages_gpu.py) and the proof that their checkers have teeth, from
oracle/siib.py and numpy alone.

  * premises, per row: the VAD gate margin, no eigenvalue of the oracle's covariance within [0.5, 2] x the 1e-10 cut (kernel and oracle keep
    the same components), the active-frame and kept-component counts the cases were chosen for (rank-deficient rows that make
    siib_quad_kernel drop row tiles, full-rank rows, a clamped replication factor, na % 4 != 0, a row with empty frame segments whose head
    and tail windows overlap);
  * siib_cases.emulate - the kernels' route in float64 numpy - passes EVERY checker on EVERY row: the derived bounds are attainable by a
    correct implementation in plain float64;
  * eight planted faults, one at a time, each fail the checker of their stage.
The oracle work (about 1 s per row, the sparse row 4 s) is shared through siib_cases.reference's cache."""
import os
import re

import numpy as np
import pytest

import siib_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
_OWN = {}


def row(key):
    """(reference, emulated buffers, own-input references) of a row, computed once"""
    if key not in _OWN:
        XL, rs = C.oracle_row(*key)
        g = C.emulate(XL, rs)
        _OWN[key] = (C.reference(*key), g, C.own_refs(g))
    return _OWN[key]


def test_constants_are_those_of_the_kernel_file():
    src = open(os.path.join(HERE, '..', 'nele_gan_amd', 'csrc', 'siib.hip')).read()
    for name, value in (('SB_J', C.J), ('SB_K', C.K_STACK), ('SB_TF', C.TF), ('SB_MMAX', C.M_MAX), ('SL_ND', C.ND_SLOTS), ('SL_CH', C.SL_CH),
                        ('SL_NSEG', C.NSEG)):
        m = re.search(r'^#define %s (\d+)' % name, src, re.M)
        assert m and int(m.group(1)) == value, name
    assert float(re.search(r'^#define SB_RELCUT (\S+)', src, re.M).group(1)) == C.RELCUT
    assert 'per = ((na + SL_NSEG - 1) / SL_NSEG + CHP - 1) / CHP * CHP' in src and 'CHP = (SL_CH / ND) * ND' in src
    assert (C.seg_per(2070, 15), C.seg_per(1918, 15), C.seg_per(2070, 29), C.seg_per(54, 15), C.seg_per(54, 29)) == (540, 495, 522, 45, 58)


@pytest.mark.parametrize('key', C.ROWS, ids=lambda k: '%s-%d' % k)
def test_premises_from_the_oracle(key):
    r = C.reference(*key)
    kept, smallest = C.check_premises(r)
    print(key, 'M rule %d, na %d, ncols %d, kept %d, smallest kept lam / lam_max %.3g, gate margin %.3g dB'
          % (r['M_rule'], r['na'], r['ncols'], kept, smallest, r['margin']))
    assert (r['na'], kept) == C.EXPECTED[key]
    assert r['ncols'] == r['na'] - 14


def test_the_cases_reach_the_paths_they_were_chosen_for():
    na = {k: v[0] for k, v in C.EXPECTED.items()}
    kept = {k: v[1] for k, v in C.EXPECTED.items()}
    assert all(kept[k] < 64 for k in C.ROWS if k[0] == 'L16000')               # rank deficient: six of seven row tiles are dropped
    assert all(kept[k] == 420 for k in C.ROWS if k[0] == 'L15871')
    assert any(n % 4 for n in na.values())
    assert {C.seg_per(n, 15) for k, n in na.items() if k[0] != 'ragged'} == {495, 540} and {C.seg_per(n, 29) for k, n in na.items() if k[0] != 'ragged'} == {522}
    assert all(3 * C.seg_per(n, 15) < n < 4 * C.seg_per(n, 15) for k, n in na.items() if k[0] != 'ragged')      # a shorter last segment
    n = na[('ragged', 3)]
    assert n == 54 and n < 2 * C.ND_SLOTS                                       # head and tail windows (29 frames each) overlap
    assert [max(0, min(n, (s + 1) * 45) - s * 45) for s in range(4)] == [45, 9, 0, 0]
    assert [max(0, min(n, (s + 1) * 58) - s * 58) for s in range(4)] == [54, 0, 0, 0]
    assert C.reference('L16000', 0)['M_rule'] == 43 and C.reference('ragged', 2)['M_rule'] == 71    # the clamp M <= 40


@pytest.mark.parametrize('key', C.ROWS, ids=lambda k: '%s-%d' % k)
def test_the_emulation_passes_every_checker(key):
    r, g, own = row(key)
    out = C.check_row(g, r, '%s-%d' % key, yx=C.is_yx(*key), own=own)
    assert set(out) == {'degraded', 'mu', 'lagp', 'C', 'S2', 'vx', 'qpart', 'score'}
    assert abs(float(g['raw']) - r['score']) <= 1e-6 * r['score']
    # what is never written reads as the fill
    assert np.all(g['lagp'][:2, :, :14].view(np.uint64) == np.uint64(0xFFFFFFFFFFFFFFFF))


CHECKERS = {
    'mu': lambda g, own, r, tag: C.check_mu(g, own, tag),
    'lagp': lambda g, own, r, tag: C.check_lagp(g, own, tag),
    'C': lambda g, own, r, tag: C.check_C(g, own, r, tag),
    'S2': lambda g, own, r, tag: C.check_S2(g, own, r, tag),
    'qpart': lambda g, own, r, tag: C.check_qpart(g, tag),
}


@pytest.mark.parametrize('key', [('ragged', 3), ('ragged', 2)], ids=lambda k: '%s-%d' % k)
@pytest.mark.parametrize('fault', sorted(C.FAULTS))
def test_a_planted_fault_fails_the_checker_of_its_stage(fault, key):
    r, g, own = row(key)
    stage = C.FAULTS[fault]
    CHECKERS[stage](g, own, r, 'sound')                                          # the same checker passes without the fault
    bad = C.emulate(g['XL'], g['rowstat'], fault=fault)
    with pytest.raises(AssertionError, match='above the bound'):
        CHECKERS[stage](bad, own, r, fault)


def test_the_own_input_moments_agree_with_a_plain_matrix_product():
    """own_refs' prefix-sum route against stack() and a float64 matrix product, at the product's own rounding level."""
    _r, g, own = row(('ragged', 2))
    from oracle import siib
    Xs = siib.stack(own['a'][0], C.K_STACK)
    Ys = siib.stack(own['a'][1], C.K_STACK)
    Xs, Ys = Xs - Xs.mean(axis=1, keepdims=True), Ys - Ys.mean(axis=1, keepdims=True)
    for pair, (P, Q) in enumerate(((Xs, Xs), (Ys, Ys), (Xs, Ys))):
        d = np.abs((P @ Q.T) - own['S'][pair].astype(np.float64))
        assert np.all(d <= C.gamma(2 * own['na']) * (np.abs(P) @ np.abs(Q).T) + 1e-300), pair


def test_the_section_list_exists_on_the_lag_product_path_only():
    """nele_metric_siib_sections is host-only: ten sections by default, NELE_ERR_UNSUPPORTED (-2) in the test library with NELE_SIIB_LAG=0,
    exactly as nele_metric_siib_clean_sections answers (the switch is read once per process: child processes)."""
    import subprocess
    import sys
    from conftest import AB_LIB, ab_env
    child = ('import ctypes, sys; lib = ctypes.CDLL(sys.argv[1]); buf = (ctypes.c_longlong * 72)(); '
             'print(lib.nele_metric_siib_sections(3, 16000, buf, 24), lib.nele_metric_siib_clean_sections(3, 16000, buf, 24))')
    for flag, want in ((1, '10 13'), (0, '-2 -2')):
        out = subprocess.run([sys.executable, '-c', child, AB_LIB], env=ab_env(NELE_SIIB_LAG=flag), stdout=subprocess.PIPE, text=True, check=True).stdout
        assert out.split() == want.split(), (flag, out)
