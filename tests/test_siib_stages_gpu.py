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

THE BACK END (everything behind the clean front end: the degraded half of spectra, masking and row statistics, siib_mu_kernel,
siib_lag_kernel, siib_assemble_kernel<0 / 1>, the eigenpairs as siib_quad_kernel and siib_final_lag_kernel use them, the score), read out
after phase 1 and again after phase 2 of the same workspace through nele_metric_siib_sections (metrics.siib_stages; C only exists between
the two).  Inputs, references, bounds and their derivations are in tests/siib_cases.py; tests/test_siib_cases_cpu.py shows on the CPU that
a float64 numpy emulation of the kernels' route meets every bound on every row and that eight planted faults do not.  Rows: the two
3-row batches above with y = clean + noise (y = x itself in row 1 of the 15 871 batch: both halves byte-equal, rho_k = 1) - 49 to 57 kept
components of 420 at 16 000 (siib_quad_kernel drops six of seven row tiles), 420 at 15 871, na % 4 != 0, a shorter last segment - and
rows 2 and 3 of siib_cases.ragged_batch() (the batch of test_siib_lag_mfma_gpu.py), run as the whole 5-row padded batch: replication rule 71 clamped to 40 (na = 1159),
and the sparse click (na = 54: segments of 45, 9, 0, 0 and 54, 0, 0, 0 frames, head and tail windows of the assembly overlap, smallest kept
lam 3.1e-10 lam_max).  The sparse row has other click samples than ragged_batch(): with the original ones an eigenvalue sits at 5.5e-11
lam_max, inside the band [0.5, 2] x 1e-10 that the premise excludes.
Each stage is checked (a) against a long-double evaluation from the kernel's own input buffers within a derived rounding bound and (b)
against the oracle within X_REL propagated.  Worst measured / bound on an MI355X over the eight rows (every test prints each figure):
  degraded XL      1.2e-14 / 2.7e-10 masked, 3.2e-14 / 1.9e-10 mean-free (last 15 frames 3.1e-14); minimum 4.3e-13, mean 3.1e-13 / 1e-10
  mu               0.019 of (na + 32) u mean|a| (5.0e-17 absolute, sparse row)
  lagp             0.12 of (terms + 4) u sum|a||b| (sparse row; 0.002 - 0.02 on the long rows); y = x: pair 1 = pair 0 bytes, L(j1, j2, D)
                   against L(j2, j1, -D) 0.002 of the bound
  C                exactly symmetric; own input 0.059 of (terms + 92) u (sum|a||b| + ncols |mu mu'|) / (ncols - 1) (2.5e-15 absolute,
                   sparse row; 0.004 - 0.02 on the long rows), oracle 1.5e-14 / 2.4e-09
  S2               own input 0.060 (Syy) and 0.044 (sym Sxy) of the same form, oracle 6.0e-12 / 8.8e-07; strict lower triangle untouched
  eigenpairs       residual against C_ref 0.0093 of n eps ||A||; vx = lam (ncols - 1) against u^T Sxx_ref u 0.0064 of twice that.
                   WORST RELATIVE vx ERROR 1.0e-07 at lam / lam_max = 4.8e-10 (sparse row; 2.2e-09 at 3.5e-08 on the full-rank rows,
                   1.7e-10 at 2.0e-07 on the rank-deficient ones): rho of that component is off by 5e-08 relative, 1e-9 of the score
  qpart            0.0016 (Syy) and 0.0026 (sym Sxy) of (420 + 64) u |u|^T |S| |u|
  score            the float64 formula on the kernel's own lam and qpart gives raw to the float32 bit in all eight rows; y = x: |rho_k - 1|
                   4.4e-16, 0.0004 of the vx bound 2 n eps lam_max / lam_k; score 3.6e-05 from 80/15 * 420 * -0.5 log2(0.4375), bound
                   2.0e-03; max |rho_k - rho_k^oracle| over well separated components
                   1.7e-12
  batch-size classes   lagp, mu, C and S2 of a row are the same bytes at B = 1, 48 and 128 (nseg = 4, 2, 1)
No kernel fault was found.  Every bound has the form the stage's derivation in siib_cases.py gives it; none had to be re-derived after a
measurement.
"""
import numpy as np
import pytest

import siib_cases as C

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

M_MAX, TF, K_STACK = C.M_MAX, C.TF, C.K_STACK
XDB_DB, X_REL, STAT_REL, LAM_REL, GATE_MARGIN_DB = C.XDB_DB, C.X_REL, C.STAT_REL, C.LAM_REL, C.GATE_MARGIN_DB
LENGTHS = C.LENGTHS
BUFFERS = ('rowstat', 'XL', 'mu', 'lagp', 'C', 'S2', 'lam', 'U', 'qpart', 'raw')


@pytest.fixture(scope='module')
def runs():
    """The clean front end after phase 3, with the oracle of siib_cases (computed once per row for the whole module)."""
    assert torch.cuda.is_available()
    from nele_gan_amd import metrics
    out = {}
    for L in LENGTHS:
        c = C.batch('L%d' % L)[0]
        out[L] = (metrics.siib_clean_stages(c), [C.reference('L%d' % L, b) for b in range(3)])
    return out


@pytest.fixture(scope='module')
def back():
    """batch name -> [(row, its buffers after phase 1 / phase 2, oracle, own-input references)] for the rows that have a reference"""
    assert torch.cuda.is_available()
    from nele_gan_amd import metrics
    out = {}
    for name in C.BATCHES:
        c, y, lengths, rows = C.batch(name)
        st = metrics.siib_stages(c, y, lengths=None if lengths is None else torch.tensor(lengths, dtype=torch.int32))
        out[name] = []
        for b in rows:
            g = {k: st[k][b] for k in BUFFERS}
            g['info1'], g['info'] = st['info1'][b], st['info'][b]
            out[name].append((b, g, C.reference(name, b), C.own_refs(g)))
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


# ---------------------------------------------------------------------------------------------------------------- the back end
def _tag(name, b):
    return '%s row %d' % (name, b)


@pytest.mark.parametrize('name', C.BATCHES)
def test_back_end_premises_and_counts(back, name):
    for b, g, r, own in back[name]:
        kept, smallest = C.check_premises(r)
        M, nt, na, status = (int(v) for v in g['info'])
        print(_tag(name, b), 'M %d (rule %d) active %d kept %d smallest kept lam / lam_max %.3g status %d' % (M, r['M_rule'], na, kept, smallest, status))
        assert (na, kept) == C.EXPECTED[(name, b)] and np.array_equal(g['info1'][:3], g['info'][:3])
        assert (M, bool(status & 1)) == (r['M'], r['M_rule'] > M_MAX) and not status & (2 | 4 | 8 | 16) and nt == len(r['xdb'])
        assert own['na'] == na == r['na']


@pytest.mark.parametrize('name', C.BATCHES)
def test_degraded_spectra_and_row_statistics(back, name):
    for b, g, r, own in back[name]:
        C.check_degraded(g, r, _tag(name, b), yx=C.is_yx(name, b))


@pytest.mark.parametrize('name', C.BATCHES)
def test_window_means(back, name):
    for b, g, r, own in back[name]:
        C.check_mu(g, own, _tag(name, b), yx=C.is_yx(name, b))


@pytest.mark.parametrize('name', C.BATCHES)
def test_lag_products(back, name):
    for b, g, r, own in back[name]:
        C.check_lagp(g, own, _tag(name, b), yx=C.is_yx(name, b))
        # slots no kernel owns keep the fill
        assert np.all(g['lagp'][:2, :, :14].view(np.uint64) == np.uint64(0xFFFFFFFFFFFFFFFF))


@pytest.mark.parametrize('name', C.BATCHES)
def test_covariance_after_phase_1(back, name):
    for b, g, r, own in back[name]:
        C.check_C(g, own, r, _tag(name, b))


@pytest.mark.parametrize('name', C.BATCHES)
def test_second_moments_of_the_degraded_signal(back, name):
    for b, g, r, own in back[name]:
        C.check_S2(g, own, r, _tag(name, b))


@pytest.mark.parametrize('name', C.BATCHES)
def test_eigenpairs_tie_to_the_reference_covariance(back, name):
    for b, g, r, own in back[name]:
        C.check_eig(g, own, r, _tag(name, b))


@pytest.mark.parametrize('name', C.BATCHES)
def test_quadratic_forms(back, name):
    for b, g, r, own in back[name]:
        C.check_qpart(g, _tag(name, b))
        kept = C.kept_of(g)
        for t0 in range(0, C.DIM, 64):                                            # a row tile without a kept component: U zero, qpart untouched
            if not kept[t0:t0 + 64].any():
                assert not g['U'][t0:t0 + 64].any(), (b, t0)
                assert np.all(g['qpart'][t0:t0 + 64].view(np.uint64) == np.uint64(0xFFFFFFFFFFFFFFFF)), (b, t0)
        assert (kept.sum() < 420 - 64) == (name != 'L15871')                      # the rank-deficient rows do drop tiles


@pytest.mark.parametrize('name', C.BATCHES)
def test_score_from_the_kernels_own_buffers(back, name):
    for b, g, r, own in back[name]:
        C.check_score(g, own, r, _tag(name, b), yx=C.is_yx(name, b))
        assert abs(float(g['raw']) - r['score']) <= 1e-4 * r['score']


def test_buffers_of_a_row_are_the_same_in_every_batch_size_class():
    """Phase 1 only (no eigensolver): one utterance at B = 1, 48 and 128 - the lag kernel deals its four frame segments to 4, 2 and 1
    workgroup groups - with a different utterance in the last row.  lagp, mu, C and S2 of row 0 are the same bytes in all three."""
    from nele_gan_amd import metrics, synth
    c, v = synth.batch(2, 4001, start=60)
    y = (c + v).astype(np.float32)
    got = {}
    for B in (1, 48, 128):
        rows = [0] * (B - 1) + [1] if B > 1 else [0]
        st = metrics.siib_stages(c[rows], y[rows], phase2=False)
        got[B] = {k: st[k][0] for k in ('mu', 'lagp', 'C', 'S2')}
    # the kernels ran: everything they own is written over the 0xFF fill (which reads as NaN)
    g = got[1]
    iu = np.triu_indices(C.DIM)
    assert np.isfinite(g['mu']).all() and np.isfinite(g['C']).all() and np.isfinite(g['S2'][:, iu[0], iu[1]]).all()
    assert np.isfinite(g['lagp'][:2, :, 14:]).all() and np.isfinite(g['lagp'][2]).all()
    for B in (48, 128):
        for k in ('lagp', 'mu', 'C', 'S2'):
            same = C.same_bytes(got[1][k], got[B][k])
            print('B = 1 against B = %d: %s %s' % (B, k, 'same bytes' if same else 'DIFFERENT'))
            assert same, (B, k)
