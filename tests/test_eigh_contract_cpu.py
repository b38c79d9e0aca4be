"""CPU: the eigensolver contract's checker (tests/eigh_contract.py) has teeth.  LAPACK's own output meets the contract on every zoo class;
outputs that are subtly wrong in the ways a batched solver goes wrong do not."""
import numpy as np
import pytest

import eigh_contract as ec


@pytest.mark.parametrize('n', (2, 3, 17, 64, 129))
def test_lapack_meets_the_contract_on_every_zoo_class(n):
    bad = []
    for name, A in ec.zoo(n, seed=7):
        r = ec.check(A, *ec.lapack(A))
        if ec.violations(r) or ec.violations(r, groups=False):
            bad.append('%s: %s' % (name, ec.violations(r)))
    assert not bad, bad


def test_lapack_meets_the_contract_on_the_siib_covariances():
    for name, A in ec.zoo(420, names=tuple('siib_%s' % w for w in ec.SIIB_INPUTS), siib=True):
        assert not ec.violations(ec.check(A, *ec.lapack(A))), name


def test_siib_covariances_have_the_spectra_the_contract_is_sized_for():
    """Periodic lengths (multiples of 200 samples) give an exact null space of 200+ eigenvalues - one group; no component SIIB keeps
    (eigenvalue > 1e-10 of the largest) is in a group."""
    for w in ec.SIIB_INPUTS:
        lam = np.linalg.eigvalsh(ec.siib_covariance(w))
        gs = ec.groups(lam, np.abs(lam).max())
        kept = lam > 1e-10 * lam.max()
        assert all(not kept[a:b].any() for a, b in gs if b - a > 1), w
        if w in (48200, 64000):
            assert max(b - a for a, b in gs) > 150, w


def _mutant_fails(A, lam, U, groups=True):
    r = ec.check(A, lam, U)
    return bool(ec.violations(r, groups=groups))


def test_two_equal_vectors_in_a_group_fail():
    A = ec.zoo(40, names=('cluster5_1e-15',))[0][1]
    lam, U = ec.lapack(A)
    a = int(np.argmin(np.abs(lam - 1.5)))
    U[a + 1] = U[a]
    assert _mutant_fails(A, lam, U)
    assert ec.check(A, lam, U)['in_group'] > 1e12


@pytest.mark.parametrize('groups', (True, False))
def test_a_vector_turned_by_1e9_toward_a_neighbour_1e2_away_fails(groups):
    n = 64
    rs = np.random.RandomState(3)
    w = np.r_[np.linspace(0.0, 0.45, 31), 0.5, 0.51, np.linspace(0.56, 1.0, n - 33)]   # 0.5 and 0.51: 1e-2 ||A|| apart, nothing closer
    A = ec.qdq(w, rs)
    lam, U = ec.lapack(A)
    i = int(np.argmin(np.abs(lam - 0.5)))
    j = int(np.argmin(np.abs(lam - 0.51)))
    th = 1e-9
    U[i] = np.cos(th) * U[i] + np.sin(th) * U[j]
    assert _mutant_fails(A, lam, U, groups)


@pytest.mark.parametrize('groups', (True, False))
@pytest.mark.parametrize('name', ('zero', 'scaled_identity', 'kron_I2_S', 'rank_n/2'))
def test_wrong_eigenvalues_of_a_repeated_spectrum_fail(name, groups):
    A = ec.zoo(64, names=(name,))[0][1]
    lam, U = ec.lapack(A)
    lam = lam + 1e-3 * max(np.abs(lam).max(), 1.0)
    assert _mutant_fails(A, lam, U, groups)


@pytest.mark.parametrize('groups', (True, False))
def test_an_eigenvalue_moved_by_2_n_eps_fails(groups):
    A = ec.zoo(64, names=('indefinite',))[0][1]
    lam, U = ec.lapack(A)
    anorm = np.abs(lam).max()
    lam[20] += 2 * 64 * ec.EPS * anorm
    assert _mutant_fails(A, lam, U, groups)
    assert ec.check(A, lam, U)['eig'] > 1.9


@pytest.mark.parametrize('groups', (True, False))
def test_rows_and_columns_swapped_fail(groups):
    A = ec.zoo(64, names=('indefinite',))[0][1]
    lam, U = ec.lapack(A)
    assert _mutant_fails(A, lam, np.ascontiguousarray(U.T), groups)


@pytest.mark.parametrize('groups', (True, False))
def test_unsorted_eigenvalues_fail(groups):
    A = ec.zoo(64, names=('indefinite',))[0][1]
    lam, U = ec.lapack(A)
    lam[[5, 6]] = lam[[6, 5]]
    U[[5, 6]] = U[[6, 5]]
    assert _mutant_fails(A, lam, U, groups)


@pytest.mark.parametrize('groups', (True, False))
def test_a_nan_in_the_vectors_fails(groups):
    A = ec.zoo(64, names=('indefinite',))[0][1]
    lam, U = ec.lapack(A)
    U[3, 17] = np.nan
    assert _mutant_fails(A, lam, U, groups)


def test_groups_follow_the_threshold():
    w = np.array([0.0, 1e-11, 2e-11, 1e-9, 0.5, 0.5 + 5e-11, 1.0])
    assert ec.groups(w, 1.0) == [(0, 3), (3, 4), (4, 6), (6, 7)]
    assert ec.groups(np.zeros(5), 0.0) == [(0, 5)]
