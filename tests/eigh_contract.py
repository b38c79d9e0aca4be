"""The accuracy contract of nele_eigh_sym_batched (include/nele_hip.h) as code: a zoo of named test matrices and a checker that
returns the contract's ratios against numpy.linalg.eigh (LAPACK, float64).  numpy only; shared by the CPU tests that prove the checker
has teeth (test_eigh_contract_cpu.py) and the GPU tests of the solver (test_eigh_gpu.py).

Notation: eps = 2^-52, ||A|| = max |lambda|, n stands for max(n, 16) (below that LAPACK's own residual exceeds n eps ||A||).  A GROUP is a maximal run of eigenvalues whose consecutive gaps are <= TAU ||A||.
    eigenvalues ascending, |lambda_j - lambda_j^LAPACK| <= n eps ||A||            ratio 'eig'       <= 1
    ||A u_j - lambda_j u_j||_2 <= n eps ||A||                                     ratio 'res'       <= 1
    (members of a group: 'eig_grp', 'res_grp' <= GROUP_EIG, the one named allowance: bisection leaves a 420-fold eigenvalue 1.0625 n eps
    ||A|| off, and a vector of an exactly repeated eigenvalue carries that error in its residual)
    | ||u_j||_2 - 1 | <= n eps                                                    ratio 'norm'      <= 1
    |u_i . u_j| <= 4 n eps inside a group                                         ratio 'in_group'  <= 4   (in units of n eps)
    |u_i . u_j| <= C_O eps ||A|| / |lambda_i - lambda_j| + 4 n eps between groups ratio 'out_group' <= C_O
    every output finite
Diagnostics with the same scaling (<= 2, resp. 2 sqrt(m) for a group of m): the angle of every ungrouped vector against LAPACK's times
its gap (Davis-Kahan), and the largest principal angle between a group's span and LAPACK's times the gap to the rest of the spectrum.
"""
import zlib

import numpy as np

EPS = 2.0 ** -52
TAU = 1e-10            # group threshold (relative to ||A||): SIIB keeps components above 1e-10 ||A||, none of them falls into a group
GROUP_EIG = 1.125      # eigenvalue / residual ratio allowed for members of a group (measured: 1.0625, identity at n = 420 and 512)
C_O = 0.375            # outside-group constant: 4x the largest ratio measured on the MI355X over the zoo (0.0936, class 'indefinite')

LIMITS = {'eig': 1.0, 'res': 1.0, 'eig_grp': GROUP_EIG, 'res_grp': GROUP_EIG, 'norm': 1.0, 'in_group': 4.0, 'out_group': C_O, 'dk': 2.0,
          'span': 2.0}


# ----------------------------------------------------------------------------------------------------------------- the zoo
def sym(A):
    """Exactly symmetric: the upper triangle mirrored."""
    return np.triu(A) + np.triu(A, 1).T


def householder_q(n, rs, k=None):
    """Product of k float64 Householder reflectors with random unit vectors (orthogonal to a few ulps)."""
    Q = np.eye(n)
    for _ in range(n if k is None else k):
        v = rs.randn(n)
        v /= np.linalg.norm(v)
        Q -= 2.0 * np.outer(Q @ v, v)
    return Q


def qdq(lam, rs):
    lam = np.asarray(lam, dtype=np.float64)
    Q = householder_q(len(lam), rs, k=min(len(lam), 24))
    return sym((Q * lam[None, :]) @ Q.T)


def wilkinson_plus(m):
    """W+_m: diagonal |k - (m - 1) / 2|, off-diagonal 1 (pairs of eigenvalues that agree to many digits)."""
    h = (m - 1) / 2.0
    return np.diag(np.abs(np.arange(m) - h)) + np.diag(np.ones(m - 1), 1) + np.diag(np.ones(m - 1), -1)


def _cluster(n, m, rel, rs):
    lam = np.sort(rs.uniform(1.0, 2.0, n))
    lam[n // 3:n // 3 + m] = 1.5 * (1.0 + rel * np.linspace(0.0, 1.0, m))
    return np.sort(lam)


def _siib_cov(which):
    import os
    import wave
    from nele_gan_amd import synth
    from oracle import siib
    if which == 'toy':
        here = os.path.dirname(os.path.abspath(__file__))
        w = wave.open(os.path.join(here, 'golden', 'toy', 'Train_Clean.wav'))
        x = np.frombuffer(w.readframes(w.getnframes()), dtype='<i2').astype(np.float32) / 32768.0
    else:
        x, _ = synth.batch(1, which, start=0)
        x = x[0]
    return siib.klt_covariance(x)


SIIB_INPUTS = ('toy', 47777, 48200, 63871, 64000)
_SIIB_CACHE = {}


def siib_covariance(which):
    """SIIB's clean covariance (n = 420) for the toy file or a synthetic utterance of length `which`, from oracle/siib.py."""
    if which not in _SIIB_CACHE:
        _SIIB_CACHE[which] = _siib_cov(which)
    return _SIIB_CACHE[which]


def zoo(n, seed=0, names=None, siib=False):
    """[(name, A)] for order n, each class seeded from (seed, n, its position).  names: only these classes.  siib: add the SIIB
    covariances (n must be 420)."""
    out = []

    def add(name, fn):
        if names is None or name in names:
            rs = np.random.RandomState([seed, n, zlib.crc32(name.encode())])        # the same matrix whichever classes are asked for
            A = fn(rs)
            assert A.shape == (n, n) and np.array_equal(A, A.T), name
            out.append((name, A))

    ar = np.arange(1, n + 1, dtype=np.float64)
    add('diag_distinct', lambda rs: np.diag(rs.permutation(ar)))
    add('diag_repeated', lambda rs: np.diag(np.repeat(ar[:(n + 2) // 3], 3)[:n]))
    add('diag_zeros', lambda rs: np.diag(np.where(np.arange(n) % 3 == 0, 0.0, ar)))
    add('zero', lambda rs: np.zeros((n, n)))
    add('identity', lambda rs: np.eye(n))
    add('scaled_identity', lambda rs: -3.25 * np.eye(n))
    add('identity_rank1', lambda rs: sym(np.eye(n) + np.outer(*(2 * [rs.randn(n) / np.sqrt(n)]))))
    add('one_large', lambda rs: qdq(np.r_[rs.uniform(0.5, 1.0, n - 1), 1e6], rs))
    add('one_small', lambda rs: qdq(np.r_[rs.uniform(0.5, 1.0, n - 1), 1e-12], rs))
    for k in (8, 15):
        add('geometric_1e%d' % k, lambda rs, k=k: qdq(np.logspace(-k, 0, n), rs))
        add('arithmetic_1e%d' % k, lambda rs, k=k: qdq(np.linspace(10.0 ** -k, 1.0, n), rs))
    add('log_uniform', lambda rs: qdq(10.0 ** rs.uniform(-12, 0, n), rs))
    for m in (2, 5, 40):
        for r in (15, 12, 9):
            if m < n:
                add('cluster%d_1e-%d' % (m, r), lambda rs, m=m, r=r: qdq(_cluster(n, m, 10.0 ** -r, rs), rs))
    if n >= 21:
        def glued(rs):
            A = np.zeros((n, n))
            for b0 in range(0, n - 20, 21):
                A[b0:b0 + 21, b0:b0 + 21] = wilkinson_plus(21)
                if b0 + 21 < n:
                    A[b0 + 20, b0 + 21] = A[b0 + 21, b0 + 20] = 1e-14
            r = n - n % 21
            A[r:, r:] = np.diag(np.arange(n - r) + 0.5)
            return A
        add('wilkinson21', lambda rs: np.pad(wilkinson_plus(21), (0, n - 21)) + np.diag(np.r_[np.zeros(21), 20.0 + np.arange(n - 21)]))
        add('wilkinson_glued', glued)
    if n % 2 == 0:
        add('kron_I2_S', lambda rs: np.kron(np.eye(2), sym(rs.randn(n // 2, n // 2))))
    for frac in (2, 4):
        def lowrank(rs, r=max(1, n // frac)):
            X = rs.randn(n, r) @ rs.randn(r, 3 * n)
            return sym(X @ X.T / (3 * n - 1))
        add('rank_n/%d' % frac, lowrank)
    add('indefinite', lambda rs: qdq(rs.uniform(-1.0, 1.0, n), rs))
    add('negative_definite', lambda rs: -qdq(10.0 ** rs.uniform(-6, 0, n), rs))
    add('scaled_1e+30', lambda rs: qdq(rs.uniform(-1.0, 1.0, n), rs) * 1e30)
    add('scaled_1e-30', lambda rs: qdq(rs.uniform(-1.0, 1.0, n), rs) * 1e-30)
    add('scaled_1e+100', lambda rs: qdq(rs.uniform(-1.0, 1.0, n), rs) * 1e100)
    add('scaled_1e-100', lambda rs: qdq(rs.uniform(-1.0, 1.0, n), rs) * 1e-100)
    if siib:
        assert n == 420
        for w in SIIB_INPUTS:
            if names is None or 'siib_%s' % w in names:
                out.append(('siib_%s' % w, siib_covariance(w)))
    return out


# ----------------------------------------------------------------------------------------------------------------- the checker
def groups(w, anorm):
    """[(start, stop)] maximal runs of the ascending eigenvalues w with consecutive gaps <= TAU anorm."""
    cut = np.nonzero(np.diff(w) > TAU * anorm)[0] + 1
    edges = np.r_[0, cut, len(w)]
    return [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]


def check(A, lam, U, ref=None):
    """Ratios of the contract for one matrix.  lam [n], U [n][n] with ROW j = eigenvector j; ref = numpy.linalg.eigh(A) if given."""
    A = np.asarray(A, dtype=np.float64)
    lam = np.asarray(lam, dtype=np.float64)
    U = np.asarray(U, dtype=np.float64)
    n = max(A.shape[0], 16)
    w, Vr = np.linalg.eigh(A) if ref is None else ref
    anorm = float(np.abs(w).max())
    sc = anorm if anorm > 0.0 else np.finfo(np.float64).tiny
    r = {'finite': bool(np.isfinite(lam).all() and np.isfinite(U).all()), 'sorted': bool(np.all(np.diff(lam) >= 0.0))}
    if not r['finite']:
        return dict(r, sorted_out=False, eig_grp=np.inf, res_grp=np.inf, eig=np.inf, res=np.inf, norm=np.inf, in_group=np.inf, out_group=np.inf, dk=np.inf, span=np.inf, groups=[])
    V = U.T
    with np.errstate(over='ignore'):                     # A = 0: any non-zero error is an infinite ratio
        err = np.abs(lam - w) / (n * EPS * sc)
        res = np.linalg.norm(A @ V - V * lam[None, :], axis=0) / (n * EPS * sc)
    r['norm'] = float(np.abs(np.linalg.norm(V, axis=0) - 1.0).max() / (n * EPS))
    gs = groups(w, anorm)
    gid = np.zeros(len(w), dtype=np.int64)
    for k, (a, b) in enumerate(gs):
        gid[a:b] = k
    same = gid[:, None] == gid[None, :]
    O = np.abs(V.T @ V)
    np.fill_diagonal(O, 0.0)
    r['in_group'] = float(O[same].max() / (n * EPS)) if same.sum() > len(w) else 0.0
    alone = np.array([b - a == 1 for a, b in gs for _ in range(b - a)])
    r['eig'] = float(err[alone].max()) if alone.any() else 0.0
    r['res'] = float(res[alone].max()) if alone.any() else 0.0
    r['eig_grp'] = float(err[~alone].max()) if (~alone).any() else 0.0
    r['res_grp'] = float(res[~alone].max()) if (~alone).any() else 0.0
    inner = gid[1:] == gid[:-1]
    r['sorted_out'] = bool(np.all(np.diff(lam)[~inner] >= 0.0))
    gap = np.abs(w[:, None] - w[None, :])
    excess = np.maximum(O - 4 * n * EPS, 0.0)
    r['out_group'] = float((excess * gap)[~same].max() / (EPS * sc)) if (~same).any() else 0.0
    # Davis-Kahan per ungrouped vector, principal angles per group (scaled by the gap to the rest of the spectrum)
    dk, span = 0.0, 0.0
    for a, b in gs:
        rest = np.r_[w[:a], w[b:]]
        g = float(np.min(np.abs(w[a:b, None] - rest[None, :]))) if len(rest) else np.inf
        if not np.isfinite(g):
            continue
        if b - a == 1:
            u = V[:, a] / np.linalg.norm(V[:, a])
            s = float(np.linalg.norm(u - np.sign(u @ Vr[:, a] or 1.0) * Vr[:, a]))
            dk = max(dk, s * g / (n * EPS * sc))
        else:
            Qu = np.linalg.svd(V[:, a:b], full_matrices=False)[0]
            P = Qu - Vr[:, a:b] @ (Vr[:, a:b].T @ Qu)
            span = max(span, float(np.linalg.norm(P, 2)) * g / (n * EPS * sc * np.sqrt(b - a)))
    r['dk'], r['span'], r['groups'] = dk, span, [b - a for a, b in gs if b - a > 1]
    return r


def violations(r, limits=None, groups=True):
    """Clauses of the contract that the ratios r break ([] = the output meets it).  groups=False leaves out only the in-group clauses -
    orthogonality and span inside a group, order inside a group - which the solver does not meet yet; eigenvalue error and residual are
    checked for every j either way."""
    lim = dict(LIMITS, **(limits or {}))
    bad = [k for k in ('finite', 'sorted' if groups else 'sorted_out') if not r[k]]
    keys = ('eig', 'res', 'eig_grp', 'res_grp', 'norm', 'out_group', 'dk') + (('in_group', 'span') if groups else ())
    bad += ['%s=%.3g>%g' % (k, r[k], lim[k]) for k in keys if not r[k] <= lim[k]]
    return bad


def lapack(A):
    """numpy.linalg.eigh in the solver's output layout: (lam, U with rows = eigenvectors)."""
    w, V = np.linalg.eigh(A)
    return w, np.ascontiguousarray(V.T)
