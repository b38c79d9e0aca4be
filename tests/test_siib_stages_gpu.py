"""GPU: the clean-signal front end of csrc/siib.hip (stages s1 - s5 and the covariance that feeds the eigensolver) against oracle/intel.py
and oracle/siib.py (float64 numpy) on the tiled clean signal, buffer by buffer, read out of the workspace after phase 3 through
nele_metric_siib_clean_sections (metrics.siib_clean_stages).  The score is a sum over 420 KLT components behind an eigen-decomposition
and hides a fault in a few frames or a band; the buffers do not.

Inputs: synth.batch(3, L, start=60) at L = 16 000 (frame-periodic: the tiled signal repeats every 80 frames, so the order statistic of
the VAD sits inside a run of exactly equal values, the spectra of later periods are copies and the masking recurrence takes its
steady-state shortcut) and L = 15 871 (no period: every frame is computed, the recurrence runs to the end).  The replication factor is
the oracle's, clamped to 40 as the kernel clamps it (row 0 at 16 000 asks for 43: status bit 1).

Bounds in force, per row:
  xdb      1e-9 dB against 10 log10(mean(frame^2) + eps), every frame of the tiled signal
  list     exact (count and frame numbers), premises asserted first from the oracle: no frame within 1e-6 dB of max_x - 40, and at
           16 000 the sorted values on both sides of the order statistic equal it exactly
  XL       1e-10 * max|X|: XL holds the log band energies AFTER forward masking and BEFORE mean removal, so it is compared (a) as it
           is with the oracle's masked X and (b) minus the kernel's own row mean (rowstat) with the oracle's mean-free X.  Both cover
           every active frame; the last Tf - 1 = 15 frames of each band, which take the shortened path m = min(Tf, n - i) of
           forward_masking, are part of it and are also reported on their own.
  rowstat  1e-10 relative: band minimum before masking, band mean after it
  lam      1e-9 * max lam against np.linalg.eigh of the oracle's covariance, components above the 1e-10 cut (loose on purpose: the
           eigensolver has its own tests, this ties the covariance that feeds it to the oracle's)
Worst errors observed on an MI355X over the six rows (every test prints its own figures): xdb 1.4e-14 dB; XL 2.0e-14 absolute against
the masked X (3.7e-15 * max|X|) and 1.9e-14 against the mean-free X, the last 15 frames no worse than the rest (1.8e-14); rowstat minimum
1.3e-15 and mean 3.2e-14 relative; lam 6.8e-13 absolute (9.5e-16 * max lam).  Lists and counts equal.  No bound had to move.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

M_MAX, TF, K_STACK = 40, 16, 15
XDB_DB, X_REL, STAT_REL, LAM_REL, GATE_MARGIN_DB = 1e-9, 1e-10, 1e-10, 1e-9, 1e-6
LENGTHS = (16000, 15871)


def oracle_clean(x):
    """Float64 reference of everything phase 3 leaves behind, for one clean row."""
    from oracle import intel, siib
    x = np.asarray(x, dtype=np.float64)
    M_rule, _ = intel.siib_replication(x)
    M = min(M_rule, M_MAX)
    xt = np.hstack([x] * M)
    fr = intel.framing(xt)
    xdb = 10 * np.log10((fr ** 2).mean(axis=1) + intel.EPS)
    n = len(xdb)
    ind = int(round(n * 0.999) - 1)
    srt = np.sort(xdb)
    thr = srt[ind] - 40
    vad = xdb > thr
    assert np.array_equal(vad, intel.get_vad(xt))
    xh = np.fft.fft(fr, n=400, axis=-1)[:, :201].T
    xh = (xh.real ** 2 + xh.imag ** 2)[:, vad]
    X0 = np.log(siib.gammatone_matrix() ** 2 @ xh + siib.EPS)
    Xm = siib.forward_masking(X0.copy(), TF)
    mean = Xm.mean(axis=1)
    Xs = siib.stack(Xm - mean[:, None], K_STACK)
    Xs = Xs - Xs.mean(axis=1, keepdims=True)
    lam = np.linalg.eigh(Xs @ Xs.T / (Xs.shape[1] - 1))[0]
    return dict(M_rule=M_rule, M=M, xdb=xdb, list=np.nonzero(vad)[0], Xm=Xm, Xc=Xm - mean[:, None], rmin=X0.min(axis=1), mean=mean, lam=lam,
                gaps=(srt[ind] - srt[ind - 1], srt[ind + 1] - srt[ind]), margin=float(np.min(np.abs(xdb - thr))))


@pytest.fixture(scope='module')
def runs():
    assert torch.cuda.is_available()
    from nele_gan_amd import metrics, synth
    out = {}
    for L in LENGTHS:
        c, _v = synth.batch(3, L, start=60)
        out[L] = (metrics.siib_clean_stages(c), [oracle_clean(c[b]) for b in range(3)])
    return out


@pytest.mark.parametrize('L', LENGTHS)
def test_premises_from_the_oracle(runs, L):
    refs = runs[L][1]
    for b, r in enumerate(refs):
        print(L, b, 'M rule %d, gaps around the order statistic %r, gate margin %.3g dB' % (r['M_rule'], r['gaps'], r['margin']))
        assert r['margin'] > GATE_MARGIN_DB
        if L % 200 == 0:
            assert r['gaps'] == (0.0, 0.0)                     # the order statistic sits inside a run of duplicates
    if L == 16000:
        assert refs[0]['M_rule'] == 43                         # the clamp M <= 40 is exercised


@pytest.mark.parametrize('L', LENGTHS)
def test_frame_powers_and_active_frame_list(runs, L):
    got, refs = runs[L]
    for b, r in enumerate(refs):
        M, nt, na, status = (int(v) for v in got['info'][b])
        assert (M, bool(status & 1)) == (r['M'], r['M_rule'] > M_MAX) and not status & (2 | 4 | 8 | 16), (b, M, status, r['M_rule'])
        assert nt == len(r['xdb']) == len(got['xdb'][b])
        e = float(np.max(np.abs(got['xdb'][b] - r['xdb'])))
        print(L, b, 'M %d frames %d active %d: xdb %.3g / %.3g dB' % (M, nt, na, e, XDB_DB))
        assert e <= XDB_DB
        assert na == len(r['list']) and np.array_equal(got['list'][b], r['list']), (b, na, len(r['list']))


@pytest.mark.parametrize('L', LENGTHS)
def test_masked_log_band_energies_and_row_statistics(runs, L):
    got, refs = runs[L]
    for b, r in enumerate(refs):
        XL, rs = got['XL'][b], got['rowstat'][b]
        assert XL.shape == r['Xm'].shape and np.isfinite(XL).all() and np.isfinite(rs).all()
        na = XL.shape[1]
        assert na > 4 * TF
        e_min = float(np.max(np.abs(rs[:, 0] - r['rmin']) / np.abs(r['rmin'])))
        e_mean = float(np.max(np.abs(rs[:, 1] - r['mean']) / np.abs(r['mean'])))
        d_m = np.abs(XL - r['Xm'])
        d_c = np.abs((XL - rs[:, 1][:, None]) - r['Xc'])
        b_m, b_c = X_REL * float(np.max(np.abs(r['Xm']))), X_REL * float(np.max(np.abs(r['Xc'])))
        print(L, b, 'active %d: masked %.3g / %.3g (last 15 frames %.3g), mean-free %.3g / %.3g (last 15 frames %.3g), min %.3g mean %.3g / %.3g'
              % (na, d_m.max(), b_m, d_m[:, -(TF - 1):].max(), d_c.max(), b_c, d_c[:, -(TF - 1):].max(), e_min, e_mean, STAT_REL))
        assert e_min <= STAT_REL and e_mean <= STAT_REL
        assert d_m.max() <= b_m and d_c.max() <= b_c
        assert d_m[:, -(TF - 1):].max() <= b_m and d_c[:, -(TF - 1):].max() <= b_c      # the shortened path of the recurrence, explicitly


@pytest.mark.parametrize('L', LENGTHS)
def test_eigenvalues_tie_the_covariance_to_the_oracle(runs, L):
    got, refs = runs[L]
    for b, r in enumerate(refs):
        good = r['lam'] > 1e-10 * r['lam'].max()
        e = float(np.max(np.abs(got['lam'][b][good] - r['lam'][good])))
        print(L, b, 'components above the cut %d of 420: lam %.3g / %.3g' % (int(good.sum()), e, LAM_REL * r['lam'].max()))
        assert (good.sum() < 420) == (L % 200 == 0)
        assert np.isfinite(got['lam'][b]).all() and e <= LAM_REL * r['lam'].max()
