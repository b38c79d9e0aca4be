"""Inputs, float64 / long-double references and checkers of the SIIB stage tests (tests/test_siib_stages_gpu.py on the device,
tests/test_siib_cases_cpu.py for the premises and for the proof that the checkers have teeth).  Plain module: numpy and oracle/ only,
nothing here touches a GPU.

A ROW's buffers are a dict in the layout of metrics.siib_stages, cut to one row: rowstat [2, 28, 2], XL [2, 28, na], mu [2, 420], lagp
[3, 4, 29, 28, 28], C [420, 420], S2 [2, 420, 420], lam [420], U [420, 420], qpart [420, 14], raw.  emulate() produces one in float64 numpy
along the kernels' route (csrc/siib.hip: segmenting with the kernel's `per`, lag sums, tail removal and the sliding update along each
diagonal, ncols mu mu', upper-triangle quadratic forms with the halved diagonal, vx from eigh's eigenvalue), optionally with one planted
fault; the checkers below take either.

Every stage is checked (a) against a long-double evaluation of the same quantity from the row's OWN input buffers (own_refs: isolates the
kernel; the bound is a rounding bound derived next to it) and, where it makes sense, (b) against the independent oracle (reference():
oracle/siib.py on the signal tiled M <= 40 times) with the front end's X_REL = 1e-10 max|X| propagated through the stage.

Notation: u = 2^-53 (unit roundoff), a_j[s] = XL[sig, j, s] - rowstat[sig, j, 1] (formed in float64 exactly as every consumer kernel forms
it, so the checkers' operands are the kernels' bit for bit), na active frames, ncols = na - 14, gamma(c) = c u / (1 - c u).  A sum of n
terms accumulated in ANY order has an error <= gamma(n - 1) sum |terms| (Higham, Accuracy and Stability, section 4.2); a product adds one
u.  The long-double references (eps < 2^-60, asserted) carry at most na 2^-63 sum |terms|, 1 / 500 of the smallest bound here.
"""
import functools

import numpy as np

from oracle import intel, siib

M_MAX, TF, K_STACK, J, DIM = 40, 16, 15, 28, 420
NSEG, ND_SLOTS, SL_CH = 4, 29, 58
RELCUT = 1e-10
XDB_DB, X_REL, STAT_REL, LAM_REL, GATE_MARGIN_DB = 1e-9, 1e-10, 1e-10, 1e-9, 1e-6
U53 = 2.0 ** -53
LD = np.longdouble
assert np.finfo(LD).eps < 2.0 ** -60, 'the references need an 80-bit (or wider) long double'
PAIRS = ((0, 0, 0, 15), (1, 1, 0, 15), (0, 1, -14, 29))        # (signal of a, signal of b, first lag D0, lags ND) of lagp pair 0, 1, 2
LENGTHS = (16000, 15871)
YX_ROW = 1                                                       # the row of the 15 871 batch whose degraded signal is the clean one
RAGGED_LENS = (64000, 63871, 9600, 64001, 40000)
SPARSE = 3                                                       # row of the sparse utterance of ragged_batch()
RAGGED_ROWS = (2, SPARSE)
SPARSE_CLICK = (0.55, -0.35, 0.2, -0.1)
# row -> (na, kept components), from the oracle (test_siib_cases_cpu.py asserts them)
EXPECTED = {('L16000', 0): (1918, 49), ('L16000', 1): (1976, 53), ('L16000', 2): (2070, 57), ('L15871', 0): (2035, 420),
            ('L15871', 1): (2008, 420), ('L15871', 2): (1990, 420), ('ragged', 2): (1159, 32), ('ragged', 3): (54, 27)}
NAN_FF = np.frombuffer(b'\xff' * 8, dtype=np.float64)[0]         # what an unwritten double of the 0xFF-filled workspace reads as


def gamma(c):
    return c * U53 / (1.0 - c * U53)


# ------------------------------------------------------------------------------------------------------------------ inputs
def ragged_batch():
    """Five utterances in one padded batch: frame-periodic (64 000), aperiodic (63 871), a short one at the largest replication factor
    (9 600: M = 40, status bit 1), a sparse one, and 40 000.
    The sparse one has fewer active frames than one 58-frame chunk of the old kernel: four non-zero samples in digital silence.  The
    replication factor follows the ACTIVE duration, so such an utterance is tiled 40 times (the cap), and it stays under 58 frames only
    while most copies give ONE active frame: 64 001 samples let the click drift by one sample per copy against the 200-sample frame
    grid, from 20 samples before a frame start to 19 behind it - the second frame that covers it sees it under the first or last few
    taps of its window, 40 dB down, except in the outermost copies.  y keeps its noise everywhere."""
    from nele_gan_amd import synth
    c, v = synth.batch(len(RAGGED_LENS), max(RAGGED_LENS), start=310)
    c[SPARSE] = 0.0
    c[SPARSE, 6380:6384] = np.float32([0.5, -0.35, 0.2, -0.1])
    y = (0.8 * c + v).astype(np.float32)
    for b, n in enumerate(RAGGED_LENS):
        c[b, n:], y[b, n:] = 0.0, 0.0
    return c, y


@functools.lru_cache(maxsize=None)
def batch(name):
    """-> (clean [B, L] float32, degraded [B, L] float32, lengths or None, rows that have a reference)"""
    from nele_gan_amd import synth
    if name == 'ragged':
        c, y = ragged_batch()
        # the sparse row with other click samples: with ragged_batch()'s own (0.5, -0.35, 0.2, -0.1) the covariance has an eigenvalue at
        # 5.5e-11 lam_max, inside the band around the 1e-10 cut that check_premises excludes; with these the nearest are 3.6e-11 and 3.1e-10
        click = np.zeros_like(c[SPARSE])
        click[6380:6384] = np.float32(SPARSE_CLICK)
        y[SPARSE] = (y[SPARSE] - np.float32(0.8) * c[SPARSE]) + np.float32(0.8) * click
        c[SPARSE] = click
        return c, y, RAGGED_LENS, RAGGED_ROWS
    L = int(name[1:])
    c, v = synth.batch(3, L, start=60)
    y = (c + v).astype(np.float32)
    if L == 15871:
        y[YX_ROW] = c[YX_ROW]
    return c, y, None, (0, 1, 2)


BATCHES = ('L16000', 'L15871', 'ragged')
ROWS = tuple(sorted(EXPECTED))


def is_yx(name, b):
    return name == 'L15871' and b == YX_ROW


# ------------------------------------------------------------------------------------------------------------------ the oracle
def _masked(fr, vad):
    """Log band energies of the active frames: before masking, after masking (oracle/siib.py's own functions)."""
    xh = np.fft.fft(fr, n=400, axis=-1)[:, :201].T
    xh = (xh.real ** 2 + xh.imag ** 2)[:, vad]
    X0 = np.log(siib.gammatone_matrix() ** 2 @ xh + siib.EPS)
    return X0, siib.forward_masking(X0.copy(), TF)


@functools.lru_cache(maxsize=None)
def reference(name, b):
    """Float64 reference of everything the kernels leave behind for row b of batch `name`: the front end (as the clean stage tests use
    it), the masked degraded signal, oracle/siib.py's stacked frames, covariance, eigenvalues and per-component rho."""
    c, yb, lengths, _rows = batch(name)
    n = c.shape[1] if lengths is None else lengths[b]
    x = np.asarray(c[b, :n], dtype=np.float64)
    y = np.asarray(yb[b, :n], dtype=np.float64)
    M_rule, _ = intel.siib_replication(x)
    M = min(M_rule, M_MAX)
    xt, yt = np.hstack([x] * M), np.hstack([y] * M)
    fr = intel.framing(xt)
    xdb = 10 * np.log10((fr ** 2).mean(axis=1) + intel.EPS)
    nt = len(xdb)
    ind = int(round(nt * 0.999) - 1)
    srt = np.sort(xdb)
    thr = srt[ind] - 40
    vad = xdb > thr
    Xs, Ys, vad2 = siib._stacked(xt, yt)
    assert np.array_equal(vad, vad2)
    X0, Xm = _masked(fr, vad)
    Y0, Ym = _masked(intel.framing(yt), vad)
    mean, ymean = Xm.mean(axis=1), Ym.mean(axis=1)
    ncols = Xs.shape[1]
    Cxx = Xs @ Xs.T / (ncols - 1)
    lam, V = np.linalg.eigh(Cxx)
    Xp, Yp = V.T @ Xs, V.T @ Ys
    vx, vy, cxy = np.sum(Xp * Xp, axis=1), np.sum(Yp * Yp, axis=1), np.sum(Xp * Yp, axis=1)
    good = lam > RELCUT * lam.max()
    rho = np.zeros_like(lam)
    rho[good] = cxy[good] / np.sqrt(vx[good] * vy[good])
    score = max(0.0, float(siib.R / K_STACK * np.sum(-0.5 * np.log2(1 - siib.RHO_P ** 2 * rho ** 2))))
    return dict(M_rule=M_rule, M=M, xdb=xdb, list=np.nonzero(vad)[0], Xm=Xm, Xc=Xm - mean[:, None], rmin=X0.min(axis=1), mean=mean,
                Ym=Ym, Yc=Ym - ymean[:, None], ymin=Y0.min(axis=1), ymean=ymean, Xs=Xs, Ys=Ys, Cxx=Cxx, lam=lam, rho=rho, good=good,
                score=score, na=int(vad.sum()), ncols=ncols,
                gaps=(srt[ind] - srt[ind - 1], srt[ind + 1] - srt[ind]), margin=float(np.min(np.abs(xdb - thr))))


def check_premises(r):
    """What the comparisons rest on, from the oracle alone: no frame at the VAD gate, no eigenvalue at the 1e-10 cut (kernel and oracle keep
    the same components), the stacked frames of _stacked are those of the masked spectra the front-end tests compare."""
    assert r['margin'] > GATE_MARGIN_DB, r['margin']
    lmax = r['lam'].max()
    near = (r['lam'] >= 0.5 * RELCUT * lmax) & (r['lam'] <= 2 * RELCUT * lmax)
    assert not near.any(), r['lam'][near] / lmax
    for Xc, Xs in ((r['Xc'], r['Xs']), (r['Yc'], r['Ys'])):
        S = siib.stack(Xc, K_STACK)
        assert np.max(np.abs(S - S.mean(axis=1, keepdims=True) - Xs)) <= 1e-12 * np.max(np.abs(Xc))
    return int(r['good'].sum()), float(r['lam'][r['good']].min() / lmax)


# ------------------------------------------------------------------------------------------------------------------ the kernels' route in numpy
def seg_per(na, nd):
    """Frames per segment of siib_lag_kernel<.., ND = nd>: ceil(na / 4) rounded up to the chunk of the kernel it replaced."""
    chp = (SL_CH // nd) * nd
    return ((na + NSEG - 1) // NSEG + chp - 1) // chp * chp


FAULTS = {                    # planted fault -> the checker that must catch it
    'tail_product_kept': 'C', 'segment_boundary_late': 'lagp', 'q_bands_swapped': 'S2', 'scale_one_over_ncols': 'C', 'mean_window_shifted': 'mu',
    'diagonal_not_halved': 'qpart', 'qpart_tile_dropped': 'qpart', 'cross_lag_sign_swapped': 'lagp'}


def emulate(XL, rowstat, fault=None):
    """The back end of csrc/siib.hip in float64 numpy, kernel by kernel, from the masked spectra XL [2, 28, na] and rowstat [2, 28, 2]."""
    assert fault is None or fault in FAULTS
    na = XL.shape[2]
    ncols = na - K_STACK + 1
    a = XL - rowstat[:, :, 1][:, :, None]
    # siib_mu_kernel: the row total minus the frames before and behind the window
    mu = np.empty((2, DIM))
    for sig in range(2):
        tot = a[sig].sum(axis=1)
        for k in range(K_STACK):
            k0 = k + 1 if fault == 'mean_window_shifted' and k < K_STACK - 1 else k
            edge = a[sig][:, :k0].sum(axis=1) + a[sig][:, k0 + ncols:].sum(axis=1)
            mu[sig, k * J:(k + 1) * J] = (tot - edge) / ncols
    # siib_lag_kernel: four frame segments, each from zero; b is zero outside [0, na)
    lagp = np.full((3, NSEG, ND_SLOTS, J, J), NAN_FF)
    for pair, (sa, sb, d0, nd) in enumerate(PAIRS):
        per = seg_per(na, nd)
        for seg in range(NSEG):
            s0, s1 = seg * per, min(na, (seg + 1) * per)
            if fault == 'segment_boundary_late' and seg == 0:
                s1 = min(na, s1 + 1)
            for D in range(d0, d0 + nd):
                lo, hi = max(s0, -D), min(s1, na - D)
                v = a[sa][:, lo:hi] @ a[sb][:, lo + D:hi + D].T if hi > lo else np.zeros((J, J))
                lagp[pair, seg, D + 14] = v
    if fault == 'cross_lag_sign_swapped':
        lagp[2] = lagp[2][:, ::-1].copy()
    # siib_assemble_kernel
    lag = (lagp[:, 0] + lagp[:, 1]) + (lagp[:, 2] + lagp[:, 3])                  # [pair, slot, j1, j2]
    eh = np.zeros((2, J, ND_SLOTS))
    et = np.zeros((2, J, ND_SLOTS))
    for q in range(ND_SLOTS):
        if q < na:
            eh[:, :, q] = a[:, :, q]
        if na - ND_SLOTS + q >= 0:
            et[:, :, q] = a[:, :, na - ND_SLOTS + q]
    C = np.zeros((DIM, DIM))
    S2 = np.full((2, DIM, DIM), NAN_FF)
    nc = float(ncols)
    scale = 1.0 / (ncols if fault == 'scale_one_over_ncols' else ncols - 1)

    def outer(p, q):              # [j1, j2] = p[j1] q[j2]
        return p[:, None] * q[None, :]

    for D in range(K_STACK):
        P = [lag[0, D + 14].copy(), lag[1, D + 14].copy()]                       # (x, x), (y, y)
        P1 = lag[2, D + 14].copy()                                               # [j1, j2] sum_t x_j1[t + k1] y_j2[t + k2]
        Q = lag[2, 14 + D].copy() if fault == 'q_bands_swapped' else lag[2, 14 - D].T.copy()    # [j1, j2] sum_t x_j2[t + k2] y_j1[t + k1]
        for i in range(14 - D):
            if fault == 'tail_product_kept' and D == 3 and i == 0:
                continue
            for s in range(2):
                P[s] -= outer(et[s][:, 15 + i], et[s][:, 15 + i + D])
            P1 -= outer(et[0][:, 15 + i], et[1][:, 15 + i + D])
            Q -= outer(et[1][:, 15 + i], et[0][:, 15 + D + i]) if fault != 'q_bands_swapped' else outer(et[0][:, 15 + i], et[1][:, 15 + i + D])
        for k1 in range(K_STACK - D):
            k2 = k1 + D
            r1, r2 = slice(k1 * J, (k1 + 1) * J), slice(k2 * J, (k2 + 1) * J)
            v = (P[0] - nc * outer(mu[0, r1], mu[0, r2])) * scale
            vy = P[1] - nc * outer(mu[1, r1], mu[1, r2])
            vxy = 0.5 * ((P1 - nc * outer(mu[0, r1], mu[1, r2])) + (Q - nc * outer(mu[1, r1], mu[0, r2])))
            if D == 0:                                                           # the kernel runs the pairs j2 <= j1 and mirrors them
                v, vy, vxy = (np.tril(m) + np.tril(m, -1).T for m in (v, vy, vxy))
            C[r1, r2] = v
            C[r2, r1] = v.T
            S2[0, r1, r2] = np.where(np.tri(J, k=-1, dtype=bool), NAN_FF, vy) if D == 0 else vy
            S2[1, r1, r2] = np.where(np.tri(J, k=-1, dtype=bool), NAN_FF, vxy) if D == 0 else vxy
            if k2 + 1 >= K_STACK:
                break
            for s in range(2):
                P[s] += outer(et[s][:, 15 + k1], et[s][:, 15 + k2]) - outer(eh[s][:, k1], eh[s][:, k2])
            P1 += outer(et[0][:, 15 + k1], et[1][:, 15 + k2]) - outer(eh[0][:, k1], eh[1][:, k2])
            if fault == 'q_bands_swapped':
                Q += outer(et[0][:, 15 + k1], et[1][:, 15 + k2]) - outer(eh[0][:, k1], eh[1][:, k2])
            else:
                Q += outer(et[1][:, 15 + k1], et[0][:, 15 + k2]) - outer(eh[1][:, k1], eh[0][:, k2])
    Cphase1 = C.copy()
    # eigensolver (rows = eigenvectors, kept components only), siib_quad_kernel, siib_final_lag_kernel
    lam, V = np.linalg.eigh(C)
    kept = lam > RELCUT * lam[-1]
    Um = np.full((DIM, DIM), NAN_FF)
    Um[kept] = V.T[kept]
    qpart = np.full((DIM, 14), NAN_FF)
    for which in range(2):
        S = np.nan_to_num(S2[which], nan=0.0)
        T = np.triu(S, 1) + (1.0 if fault == 'diagonal_not_halved' else 0.5) * np.diag(np.diag(S))
        for t in range(7):
            cols = slice(64 * t, min(DIM, 64 * t + 64))
            qpart[kept, 7 * which + t] = 2.0 * np.sum((Um[kept] @ T[:, cols]) * Um[kept][:, cols], axis=1)
    if fault == 'qpart_tile_dropped':
        qpart[kept, 6] = 0.0
    raw = score_from(lam, qpart, ncols)
    return dict(rowstat=rowstat, XL=XL, mu=mu, lagp=lagp, C=Cphase1, S2=S2, lam=lam, U=Um, qpart=qpart, raw=np.float32(raw))


def score_from(lam, qpart, ncols):
    """siib_final_lag_kernel's formula in float64 -> score"""
    return _score_rho(lam, qpart, ncols)[0]


def _score_rho(lam, qpart, ncols):
    """-> (score, rho [420] with zeros for the components that are cut)"""
    kept = lam > RELCUT * lam.max()
    vy = np.zeros(DIM)
    cxy = np.zeros(DIM)
    for t in range(7):
        vy[kept] += qpart[kept, t]
        cxy[kept] += qpart[kept, 7 + t]
    rho = np.zeros(DIM)
    rho[kept] = cxy[kept] / np.sqrt(lam[kept] * float(ncols - 1) * vy[kept])
    with np.errstate(invalid='ignore'):                  # a planted fault may push |rho| past 4 / 3
        info = _info(rho)
    return max(0.0, 80.0 / 15.0 * float(np.sum(info[kept]))), rho


# ------------------------------------------------------------------------------------------------------------------ own-input references
def own_refs(g):
    """Long-double second moments from a row's own XL and rowstat: window means, lag products over all valid frames, and the three
    moment matrices Sxx, Syy, Sxy [420, 420] = sum_{t < ncols} a[t + k1] b[t + k2] - ncols mu mu', each with the sum of the absolute
    products its bound scales with.  Route: prefix sums of the products a_j1[s] b_j2[s + D] along s per lag D, a window sum as the
    difference of two prefixes - neither the kernel's route (lag sum minus tails, sliding update) nor the oracle's (matrix product)."""
    XL, rs = g['XL'], g['rowstat']
    na = XL.shape[2]
    ncols = na - K_STACK + 1
    a = XL - rs[:, :, 1][:, :, None]
    aL, ab = a.astype(LD), np.abs(a)
    mu = np.stack([np.concatenate([aL[s][:, k:k + ncols].sum(axis=1) / LD(ncols) for k in range(K_STACK)]) for s in range(2)])
    lagL = np.zeros((3, ND_SLOTS, J, J), dtype=LD)
    lagA = np.zeros((3, ND_SLOTS, J, J))
    nterm = np.zeros((3, ND_SLOTS))
    S = np.zeros((3, DIM, DIM), dtype=LD)
    SA = np.zeros((3, DIM, DIM))                      # sum over ALL valid frames of |a_j1[s]| |b_j2[s + D]| for the entry's lag
    NT = np.zeros((3, DIM, DIM))                      # the number of those frames, na - |D|
    for pair, (sa, sb, d0, nd) in enumerate(PAIRS):
        for D in range(d0, d0 + nd):
            lo, hi = max(0, -D), min(na, na - D)
            p = aL[sa][:, None, lo:hi] * aL[sb][None, :, lo + D:hi + D]
            cs = np.concatenate([np.zeros((J, J, 1), dtype=LD), np.cumsum(p, axis=2)], axis=2)
            lagL[pair, D + 14] = cs[:, :, -1]
            lagA[pair, D + 14] = ab[sa][:, lo:hi] @ ab[sb][:, lo + D:hi + D].T
            nterm[pair, D + 14] = hi - lo
            for k1 in range(max(0, -D), min(K_STACK, K_STACK - D)):
                k2 = k1 + D
                r1, r2 = slice(k1 * J, (k1 + 1) * J), slice(k2 * J, (k2 + 1) * J)
                S[pair, r1, r2] = cs[:, :, k1 + ncols - lo] - cs[:, :, k1 - lo] - LD(ncols) * mu[sa][r1][:, None] * mu[sb][r2][None, :]
                SA[pair, r1, r2] = lagA[pair, D + 14]
                NT[pair, r1, r2] = hi - lo
        if sa == sb:                                  # lags D >= 0 fill the upper block triangle: mirror it
            blk = (np.arange(DIM) // J)
            low = blk[:, None] > blk[None, :]
            S[pair][low] = S[pair].T[low]
            SA[pair][low] = SA[pair].T[low]
            NT[pair][low] = NT[pair].T[low]
    return dict(na=na, ncols=ncols, a=a, mu=mu, meanabs=ab.mean(axis=2), lagL=lagL, lagA=lagA, nterm=nterm, S=S, SA=SA, NT=NT)


class Report(list):
    """(label, measured, bound) triples of one checker; ok() prints every ratio and asserts them all."""

    def add(self, label, measured, bound):
        m, b = np.asarray(measured, dtype=np.float64), np.asarray(bound, dtype=np.float64)
        assert m.shape == b.shape or b.ndim == 0
        bad = ~(m <= b)
        with np.errstate(divide='ignore', invalid='ignore'):
            ratio = np.where(b > 0, m / b, np.where(m == 0, 0.0, np.inf))
        i = np.unravel_index(int(np.argmax(np.where(np.isnan(ratio), np.inf, ratio))), m.shape) if m.ndim else ()
        self.append((label, float(m[i]), float(np.broadcast_to(b, m.shape)[i]), int(bad.sum())))

    def ok(self, tag):
        for label, m, b, nbad in self:
            print('%s %s: measured %.3g / bound %.3g (%.3g)%s' % (tag, label, m, b, m / b if b > 0 else float(m > 0),
                                                                 '  <-- %d entries above' % nbad if nbad else ''))
        bad = [label for label, _m, _b, nbad in self if nbad]
        assert not bad, '%s: above the bound: %s' % (tag, bad)
        return self


def same_bytes(p, q):
    return p.shape == q.shape and np.array_equal(np.ascontiguousarray(p).view(np.uint64), np.ascontiguousarray(q).view(np.uint64))


# ------------------------------------------------------------------------------------------------------------------ the checkers
def check_degraded(g, r, tag, yx=False):
    """Stage 1: XL[1] and rowstat[1] against the oracle's masked degraded spectra on the CLEAN signal's active list - the comparisons and
    bounds of the clean half (X_REL max|Y| for the masked values as they are and minus the kernel's own row mean; STAT_REL for the band
    minimum and mean), the last Tf - 1 = 15 frames (the shortened path of the masking recurrence) also on their own."""
    XL, rs = g['XL'][1], g['rowstat'][1]
    assert XL.shape == r['Ym'].shape and np.isfinite(XL).all() and np.isfinite(rs).all()
    rep = Report()
    d_m, d_c = np.abs(XL - r['Ym']), np.abs((XL - rs[:, 1][:, None]) - r['Yc'])
    b_m, b_c = X_REL * float(np.max(np.abs(r['Ym']))), X_REL * float(np.max(np.abs(r['Yc'])))
    rep.add('masked Y', d_m.max(), b_m)
    rep.add('masked Y, last 15 frames', d_m[:, -(TF - 1):].max(), b_m)
    rep.add('mean-free Y', d_c.max(), b_c)
    rep.add('mean-free Y, last 15 frames', d_c[:, -(TF - 1):].max(), b_c)
    rep.add('band minimum (relative)', np.max(np.abs(rs[:, 0] - r['ymin']) / np.abs(r['ymin'])), STAT_REL)
    rep.add('band mean (relative)', np.max(np.abs(rs[:, 1] - r['ymean']) / np.abs(r['ymean'])), STAT_REL)
    if yx:
        assert same_bytes(g['XL'][1], g['XL'][0]) and same_bytes(g['rowstat'][1], g['rowstat'][0]), 'y = x: the degraded half differs from the clean one'
    return rep.ok(tag)


def check_mu(g, own, tag, yx=False):
    """Stage 2: the window means against mean_{t < ncols} a_j[t + k] in long double.
    Bound (na + 32) u mean|a_j| (mean over the row's na frames).  The kernel forms (T - e) / ncols: T the row total over na frames - 256
    thread-strided partial sums of ceil(na / 256) terms, then a reduction tree of at most 16 levels, so no term passes through more than
    ceil(na / 256) + 16 additions - e the <= 14 frames outside the window (<= 14 additions), one subtraction, one division.  Every
    partial sum is bounded by sum|a|, so the error is <= gamma(ceil(na / 256) + 32) sum|a| / ncols = gamma(..) (na / ncols) mean|a|, below
    (na + 32) u mean|a| whenever (ceil(na / 256) + 32) na <= (na + 31) ncols - true from na = 46 on, asserted for the row."""
    na, ncols = own['na'], own['ncols']
    assert (-(-na // 256) + 32) * na <= (na + 31) * ncols and np.isfinite(g['mu']).all()
    rep = Report()
    bound = (na + 32) * U53 * np.tile(own['meanabs'], (1, K_STACK))
    rep.add('mu', np.abs(g['mu'].astype(LD) - own['mu']).astype(np.float64), bound)
    if yx:
        assert same_bytes(g['mu'][1], g['mu'][0]), 'y = x: the window means of the two halves differ'
    return rep.ok(tag)


def lag_combined(lagp):
    """(s0 + s1) + (s2 + s3) in float64, as siib_assemble_kernel adds the four segments"""
    return (lagp[:, 0] + lagp[:, 1]) + (lagp[:, 2] + lagp[:, 3])


def check_lagp(g, own, tag, yx=False):
    """Stage 3: the lag products, four segments combined, against sum_s a_j1[s] b_j2[s + D] over all valid s in long double.
    Bound (terms + 4) u sum_s |a_j1[s]| |b_j2[s + D]|: `terms` products (u each) accumulated in `terms` - 1 additions spread over four
    segments plus the 3 additions that combine them - gamma(terms + 3) on the sum of absolute products by the any-order bound; the
    padding products the kernel also adds are exact zeros.  (terms + 4) u covers gamma(terms + 3) as long as terms < 2^25.)
    y = x: pair 1 is pair 0 byte for byte, and the cross products L(j1, j2, D) and L(j2, j1, -D) - the same products summed from other
    segment starts - agree within that same bound (two values each within it of the truth could differ by twice as much; one suffices on
    every row, so the tighter figure stands)."""
    lp = g['lagp']
    rep = Report()
    for pair, (_sa, _sb, d0, nd) in enumerate(PAIRS):
        own_slots = lp[pair][:, d0 + 14:d0 + 14 + nd]
        assert np.isfinite(own_slots).all(), 'pair %d: a segment slot the kernel owns is not finite' % pair
        for seg in range(NSEG):
            if seg * seg_per(own['na'], nd) >= own['na']:
                assert not own_slots[seg].any(), 'pair %d: empty segment %d does not hold zeros' % (pair, seg)
        got = lag_combined(lp[pair:pair + 1])[0][d0 + 14:d0 + 14 + nd]
        ref = own['lagL'][pair][d0 + 14:d0 + 14 + nd]
        bound = (own['nterm'][pair][d0 + 14:d0 + 14 + nd, None, None] + 4) * U53 * own['lagA'][pair][d0 + 14:d0 + 14 + nd]
        rep.add('pair %d' % pair, np.abs(got.astype(LD) - ref).astype(np.float64), bound)
    if yx:
        assert same_bytes(lp[1][:, 14:], lp[0][:, 14:]), 'y = x: pair (y, y) differs from pair (x, x)'
        c2 = lag_combined(lp[2:3])[0]
        mirror = c2[::-1].transpose(0, 2, 1)                                   # [D + 14, j1, j2] <- L(j2, j1, -D)
        rep.add('y = x: L(j1, j2, D) against L(j2, j1, -D)', np.abs(c2 - mirror), (own['nterm'][2][:, None, None] + 4) * U53 * own['lagA'][2])
    return rep.ok(tag)


def moment_bound(own, pair):
    """Rounding bound of one entry of Sxx, Syy or Sxy as siib_assemble_kernel forms it from lagp and XL, against the long-double value:
        c u (A + ncols |mu_a mu_b|),        c = terms + 92,
    A = sum over ALL valid frames of |a_j1[s]| |b_j2[s + D]| (it contains every product the kernel touches: the lag sum's, the tail
    products' and the window updates' are all products of frames D apart), terms = na - |D| of them.  c counts the roundings an entry
    passes through: terms + 4 for the combined lag sum (check_lagp), 28 for at most 14 tail removals (a product and a subtraction each),
    56 for at most 14 window moves = 28 updates (a product and an addition / subtraction each), 4 for the correction ncols mu mu' (two
    products, the subtraction) and the final scaling or halving; every intermediate is bounded by A + ncols |mu mu'|.
    The kernel's correction uses its own window means, the reference exact ones; the means have their own check (check_mu) and their
    error is not charged a second time here."""
    ncols = own['ncols']
    sa, sb = PAIRS[pair][0], PAIRS[pair][1]
    ma, mb = np.abs(own['mu'][sa]).astype(np.float64), np.abs(own['mu'][sb]).astype(np.float64)
    return (own['NT'][pair] + 92) * U53 * (own['SA'][pair] + ncols * np.outer(ma, mb))


def _propagated(r, pair, ncols):
    """Oracle check (b): what the front end's tolerance allows between the kernel's moments and the oracle's.  Every mean-free value
    a_j[s] is within d = X_REL max|Xc| of the oracle's (the front-end test asserts exactly that), a window mean of them too, so a stacked,
    window-mean-free entry xs is within 2 d; then |sum_t xs xs' - sum_t xs° xs°'| <= sum_t (|xs°| 2 d' + |xs°'| 2 d + 4 d d'), plus the
    oracle's own float64 product ncols u |Xs| |Xs'|^T."""
    dx, dy = X_REL * float(np.max(np.abs(r['Xc']))), X_REL * float(np.max(np.abs(r['Yc'])))
    P, Q, dp, dq = ((r['Xs'], r['Xs'], dx, dx), (r['Ys'], r['Ys'], dy, dy), (r['Xs'], r['Ys'], dx, dy))[pair]
    sp, sq = np.abs(P).sum(axis=1), np.abs(Q).sum(axis=1)
    return 2 * dq * sp[:, None] + 2 * dp * sq[None, :] + 4 * dp * dq * ncols + ncols * U53 * (np.abs(P) @ np.abs(Q).T)


def check_C(g, own, r, tag):
    """Stage 4: C after phase 1 - exactly symmetric; (a) entrywise against Sxx / (ncols - 1) rebuilt in long double from the row's own XL,
    bound moment_bound / (ncols - 1); (b) against the oracle's Xs Xs^T / (ncols - 1) with _propagated added."""
    C, ncols = g['C'], own['ncols']
    assert np.isfinite(C).all() and np.array_equal(C, C.T), 'C is not exactly symmetric'
    rep = Report()
    ba = moment_bound(own, 0) / (ncols - 1)
    rep.add('C own input', np.abs(C.astype(LD) - own['S'][0] / LD(ncols - 1)).astype(np.float64), ba)
    if r is not None:
        rep.add('C oracle', np.abs(C - r['Cxx']), ba + _propagated(r, 0, ncols) / (ncols - 1))
    return rep.ok(tag)


def check_S2(g, own, r, tag):
    """Stage 5: the upper triangles of Syy and (Sxy + Sxy^T) / 2 the same way (the symmetric part: half the sum of two entries' bounds and
    one more rounding for the addition); the strict lower triangle still holds the 0xFF the workspace was filled with."""
    S2, ncols = g['S2'], own['ncols']
    iu, il = np.triu_indices(DIM), np.tril_indices(DIM, -1)
    rep = Report()
    bxy = moment_bound(own, 2)
    sym = (own['S'][2] + own['S'][2].T) / LD(2)
    bsym = 0.5 * (bxy + bxy.T) + U53 * np.abs(sym).astype(np.float64)
    refs = ((own['S'][1], moment_bound(own, 1), None if r is None else (r['Ys'] @ r['Ys'].T, _propagated(r, 1, ncols))),
            (sym, bsym, None if r is None else (0.5 * (r['Xs'] @ r['Ys'].T + r['Ys'] @ r['Xs'].T),
                                                  0.5 * (_propagated(r, 2, ncols) + _propagated(r, 2, ncols).T))))
    for which, (ref, ba, orc) in enumerate(refs):
        name = ('Syy', 'sym(Sxy)')[which]
        got = S2[which]
        assert np.isfinite(got[iu]).all(), name
        assert np.all(got[il].view(np.uint64) == np.uint64(0xFFFFFFFFFFFFFFFF)), '%s: the strict lower triangle was written' % name
        rep.add('%s own input' % name, np.abs(got[iu].astype(LD) - ref[iu]).astype(np.float64), ba[iu])
        if orc is not None:
            rep.add('%s oracle' % name, np.abs(got[iu] - orc[0][iu]), (ba + orc[1])[iu])
    return rep.ok(tag)


def kept_of(g):
    lam = g['lam']
    assert np.isfinite(lam).all()
    return lam > RELCUT * lam.max()


def check_eig(g, own, r, tag):
    """Stage 6, tie only: for the kept components ||C_ref u_k - lam_k u_k||_2 within the residual limit of tests/eigh_contract.py
    (n eps ||A||, n = 420, eps = 2^-52, ||A|| = max lam) with C_ref the long-double own-input covariance rounded to float64, and
    |lam_k (ncols - 1) - u_k^T Sxx_ref u_k| within twice that limit times (ncols - 1): u^T C u - lam = u^T (C u - lam u) + lam (1 - |u|^2),
    a residual and a norm defect of n eps each.  Returns (worst relative error of vx = lam_k (ncols - 1), its lam_k / lam_max)."""
    import eigh_contract as E
    lam, Um, ncols = g['lam'], g['U'], own['ncols']
    kept = kept_of(g)
    if r is not None:
        assert np.array_equal(kept, r['good']), 'the kernel keeps %d components, the oracle %d' % (kept.sum(), r['good'].sum())
    Uk = Um[kept]
    assert np.isfinite(Uk).all(), 'an eigenvector of a kept component is not finite'
    limit = E.LIMITS['res'] * max(DIM, 16) * E.EPS * float(np.abs(lam).max())
    Cref = (own['S'][0] / LD(ncols - 1)).astype(np.float64)
    res = np.linalg.norm(Uk @ Cref - lam[kept][:, None] * Uk, axis=1)
    UL = Uk.astype(LD)
    vx_ref = np.sum((UL @ own['S'][0]) * UL, axis=1)
    vx = lam[kept].astype(LD) * LD(ncols - 1)
    evx = np.abs(vx - vx_ref).astype(np.float64)
    rep = Report()
    rep.add('residual against C_ref', res, limit)
    rep.add('vx = lam (ncols - 1) against u^T Sxx_ref u', evx, 2 * limit * (ncols - 1))
    rel = evx / np.abs(vx_ref).astype(np.float64)
    k = int(np.argmax(rel))
    print('%s worst relative vx error %.3g at lam / lam_max = %.3g (%d kept)' % (tag, rel[k], lam[kept][k] / lam.max(), kept.sum()))
    rep.ok(tag)
    return float(rel[k]), float(lam[kept][k] / lam.max())


def check_qpart(g, tag):
    """Stage 7: for the kept components the sums of the 7 + 7 partials against u_k^T S u_k in long double from the row's own U and own S2
    (upper triangle mirrored).  Bound c u |u|^T |S| |u| with c = 420 + 64: a partial is a product over <= 420 rows of S accumulated on
    the matrix cores and a sum over the 64 columns of its tile (products, the in-lane sum of four, the 16-lane reduction), each entry of S
    and of u entering once or (halved diagonal: exact) twice; the seven partials are added here in long double."""
    kept = kept_of(g)
    Uk, qp = g['U'][kept], g['qpart'][kept]
    assert np.isfinite(qp).all(), 'a partial of a kept component is not finite'
    UL, UA = Uk.astype(LD), np.abs(Uk)
    rep = Report()
    for which in range(2):
        S = np.triu(g['S2'][which]) + np.triu(g['S2'][which], 1).T
        ref = np.sum((UL @ S.astype(LD)) * UL, axis=1)
        got = qp[:, 7 * which:7 * which + 7].astype(LD).sum(axis=1)
        bound = (DIM + 64) * U53 * np.sum((UA @ np.abs(S)) * UA, axis=1)
        rep.add(('u^T Syy u', 'u^T sym(Sxy) u')[which], np.abs(got - ref).astype(np.float64), bound)
    return rep.ok(tag)


def _info(rho):
    """bits of one component, siib_final_lag_kernel's formula"""
    return -0.5 * np.log2(1.0 - 0.5625 * rho * rho)


def check_score(g, own, r, tag, yx=False):
    """Stage 8: siib_final_lag_kernel's formula in float64 on the row's own lam and qpart, rounded to float32, equals raw to one float32
    ulp (the kernel adds the components in another order: a few float64 ulps).  y = x: every kept rho_k is 1 within e_k = E_k / vx_k,
    E_k = 2 limit (ncols - 1) the vx bound of check_eig and vx_k = lam_k (ncols - 1) (vy = cxy = vx in exact arithmetic and
    rho = cxy / sqrt(vx vy)).  The bits of a component grow with |rho| and are convex in it, so |I(rho_k) - I(1)| <= I(1 + e_k) - I(1)
    and the score is 80 / 15 * kept * (-0.5 log2(0.4375)) within 80 / 15 * sum_k (I(1 + e_k) - I(1)) and one float32 ulp for raw's own
    rounding.  Reported, not asserted: max_k |rho_k - rho_k^oracle| over the components whose gap to both neighbours exceeds 1e-6 lam_max
    (elsewhere the basis is not unique)."""
    import eigh_contract as E
    ncols = own['ncols']
    val, rho = _score_rho(g['lam'], g['qpart'], ncols)
    raw = np.float32(g['raw'])
    rep = Report()
    rep.add('raw against the float64 formula (float32 ulps)', abs(float(raw) - float(np.float32(val))) / float(np.spacing(np.float32(val))), 1.0)
    kept = kept_of(g)
    if r is not None:
        lam = r['lam']
        gap = np.minimum(np.diff(lam, prepend=-np.inf), np.diff(lam, append=np.inf))
        sel = kept & r['good'] & (gap > 1e-6 * lam.max())
        d = np.abs(np.abs(rho[sel]) - np.abs(r['rho'][sel]))
        print('%s score %.6f oracle %.6f; max |rho - rho_oracle| %.3g over %d well separated components of %d kept'
              % (tag, float(raw), r['score'], d.max() if d.size else 0.0, int(sel.sum()), int(kept.sum())))
    if yx:
        limit = E.LIMITS['res'] * max(DIM, 16) * E.EPS * float(np.abs(g['lam']).max())
        ek = 2 * limit * (ncols - 1) / (g['lam'][kept] * (ncols - 1))
        assert ek.max() < 1.0 / 3.0, 'the vx bound leaves rho of a kept component outside the formula\'s domain'
        rep.add('y = x: |rho_k - 1|', np.abs(rho[kept] - 1.0), ek)
        ideal = 80.0 / 15.0 * int(kept.sum()) * float(_info(1.0))
        rep.add('y = x: score against 80/15 * kept * -0.5 log2(0.4375)', abs(float(raw) - ideal),
                80.0 / 15.0 * float(np.sum(_info(1.0 + ek) - _info(1.0))) + float(np.spacing(np.float32(ideal))))
    return rep.ok(tag)


def check_row(g, r, tag, yx=False, own=None):
    """Every stage of one row, in order -> {stage: Report}, 'vx': (worst relative vx error, its lam / lam_max)"""
    own = own_refs(g) if own is None else own
    out = {'degraded': check_degraded(g, r, tag, yx), 'mu': check_mu(g, own, tag, yx), 'lagp': check_lagp(g, own, tag, yx),
           'C': check_C(g, own, r, tag), 'S2': check_S2(g, own, r, tag)}
    out['vx'] = check_eig(g, own, r, tag)
    out['qpart'] = check_qpart(g, tag)
    out['score'] = check_score(g, own, r, tag, yx)
    return out


def oracle_row(name, b):
    """The masked spectra and row statistics of the oracle in the layout of a row's XL / rowstat (what emulate() starts from)."""
    r = reference(name, b)
    XL = np.stack([r['Xm'], r['Ym']])
    rowstat = np.stack([np.stack([r['rmin'], r['mean']], axis=1), np.stack([r['ymin'], r['ymean']], axis=1)])
    return XL, rowstat
