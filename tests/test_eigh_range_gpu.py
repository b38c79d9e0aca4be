"""GPU: nele_eigh_sym_batched_range (eigenvectors on request) against nele_eigh_sym_batched on matrices of known rank.

A = Q diag(lam) Q^T in float64 with n - rank zero eigenvalues (computed: a few 1e-17 ||A||, eight orders below the cut 1e-10 ||A||), one
rank per batch slot.  The ranged call must give the full call's eigenvalues and, from the 64-vector block that holds the first kept
component upwards, the full call's eigenvectors to the bit; the blocks below are zero; kept_first is the count the host makes from the
returned eigenvalues.  The contract (tests/eigh_contract.py) is checked on the kept vectors with LAPACK's vectors standing in for the
skipped ones."""
import numpy as np
import pytest

import eigh_contract as ec

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
REL_CUT = 1e-10


def matrix(n, cut, seed):
    """n x n, the lowest `cut` eigenvalues zero, the others spread over [0.5, 2]; cut = n: the zero matrix."""
    if cut >= n:
        return np.zeros((n, n))
    rs = np.random.RandomState(seed)
    lam = np.r_[np.zeros(cut), np.sort(rs.uniform(0.5, 2.0, n - cut))]
    return ec.qdq(lam, rs)


def both(As):
    from nele_gan_amd import metrics as mt
    A = torch.from_numpy(np.ascontiguousarray(As)).cuda()
    lam0, U0 = mt.eigh_batched(A)
    lam0, U0 = lam0.cpu().numpy(), U0.cpu().numpy()
    lam1, U1, kf = mt.eigh_batched_range(A, REL_CUT, poison=True)
    return lam0, U0, lam1.cpu().numpy(), U1.cpu().numpy(), kf.cpu().numpy()


def check_ranged(As, cuts):
    n = As.shape[1]
    lam0, U0, lam1, U1, kf = both(As)
    assert np.array_equal(lam0, lam1)
    for b, cut in enumerate(cuts):
        host = n - int((lam1[b] > REL_CUT * lam1[b, n - 1]).sum())
        assert host == cut and kf[b] == host, (b, cut, host, kf[b])
        blk = 64 * (cut // 64) if cut < n else n                      # first row of the first block with a kept vector
        assert np.array_equal(U1[b, blk:], U0[b, blk:]), b            # kept vectors (and the cut ones of their block): the same bits
        assert np.all(U1[b, :blk] == 0.0), b                          # skipped blocks: zero, not what the buffer held
        # the contract on the kept vectors: LAPACK's vectors in place of the skipped ones
        w, Vr = ec.lapack(As[b])
        Uc = U1[b].copy()
        Uc[:blk] = Vr[:blk]
        v = ec.violations(ec.check(As[b], lam1[b], Uc), groups=False)
        assert not v, (b, cut, v)


# n = 130: three 64-blocks, the last partial.  Cuts: on a block boundary (64), inside a block (70), nowhere (0), everything but one
# vector (129), the zero matrix (130); each batch turned through every slot.
@pytest.mark.parametrize('cuts', [(64, 70, 0), (70, 0, 64), (0, 64, 70), (129, 130, 64), (130, 128, 129)])
def test_n130_cut_on_and_inside_blocks(cuts):
    As = np.stack([matrix(130, c, 10 + c) for c in cuts])
    check_ranged(As, cuts)


# n = 64: a single block, computed whole unless everything is cut
@pytest.mark.parametrize('cuts', [(0, 63, 64), (10, 64, 0)])
def test_n64_single_block(cuts):
    As = np.stack([matrix(64, c, 20 + c) for c in cuts])
    check_ranged(As, cuts)


def test_n420_rank_209_runs_the_siib_instantiation():
    """SIIB's order: the 27-tile back-transformation, seven blocks of which the first three are cut (211 = 420 - 209 >= 192)."""
    cuts = (211, 0)
    As = np.stack([matrix(420, c, 30 + c) for c in cuts])
    check_ranged(As, cuts)


def test_no_cut_requested_is_the_full_call():
    from nele_gan_amd import metrics as mt
    A = torch.from_numpy(np.stack([matrix(130, c, 40 + c) for c in (70, 130, 0)])).cuda()
    lam0, U0 = mt.eigh_batched(A)
    lam1, U1, kf = mt.eigh_batched_range(A, -1.0, poison=True)
    assert torch.equal(lam0, lam1) and torch.equal(U0, U1) and not kf.any()
