"""GPU: every stage of csrc/estoi.hip against oracle/estoi.py (float64 numpy / scipy), row by row, read out of the workspace through
nele_metric_estoi_sections (metrics.estoi_stages).  The final score is a mean over segments and hides a fault in a few frames; the stages
do not.  Cases and their premises: tests/estoi_cases.py, tests/test_estoi_cases_cpu.py.

Bounds in force (the constants below) and where they come from:
  xr    1e-12 * max|input|   117 float64 products per output, sum |h| ~ 2.35 per phase: rounding < 1e-13 * max|input|
  en    1e-9 dB              256 float64 squares, sqrt, log10
  keep, nkept  exact         (no frame of any case within 1e-6 dB of the gate: test_estoi_cases_cpu.py)
  tob   1e-10 * max of the row's reference plane     512-point float64 FFT, <= 45 bins per band
  dseg  1e-9 absolute        two normalisations of 15 x 30 values
  raw   1.2e-7 relative + 1e-8 absolute against float32(oracle)   one float32 rounding on either side
A NaN of the oracle (digital silence) must be a NaN of the kernel at the same place; nothing is dropped from a comparison.
Worst errors observed on an MI355X over all cases and ragged rows (every test prints its own figures): xr 4.7e-16 * max|input|,
en 5.7e-14 dB (gapped_64000), tob 4.7e-16 of the plane's maximum, dseg 2.8e-16, raw bit-equal to float32(oracle) in every row; the rows
of digital silence, 100 and 0 samples agree exactly.  No bound had to move.
"""
import numpy as np
import pytest

import estoi_cases as C

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

XR_REL, EN_DB, TOB_REL, DSEG_ABS, RAW_REL, RAW_ABS = 1e-12, 1e-9, 1e-10, 1e-9, 1.2e-7, 1e-8


@pytest.fixture(scope='module')
def mt():
    assert torch.cuda.is_available()
    from nele_gan_amd import metrics
    return metrics


def same_nan(got, ref):
    return np.array_equal(np.isnan(got), np.isnan(ref))


def err(got, ref):
    """largest |got - ref| where the reference is a number (NaN places are compared by same_nan); 0 for an empty stage"""
    ok = ~np.isnan(ref)
    return float(np.max(np.abs(got[ok] - ref[ok]))) if ok.any() else 0.0


def compare(tag, x, y, raw, st, b, ref):
    """Row b of estoi_stages' output against the oracle's stages of (x, y); prints each figure with its bound, then asserts."""
    got = {k: st[k][b] for k in ('xr', 'en', 'keep', 'tob', 'dseg')}
    shapes = {k: (got[k].shape, ref[k].shape) for k in got}
    assert all(g == r for g, r in shapes.values()), (tag, shapes)
    assert int(st['nkept'][b]) == ref['nkept'], (tag, int(st['nkept'][b]), ref['nkept'])
    assert np.array_equal(got['keep'], ref['keep']), tag
    fig = {}
    for p, s in enumerate((x, y)):
        amax = float(np.max(np.abs(s))) if len(s) else 0.0
        fig['xr[%d]' % p] = (err(got['xr'][p], ref['xr'][p]), XR_REL * amax)
        tmax = float(np.max(ref['tob'][p])) if ref['tob'][p].size else 0.0
        fig['tob[%d]' % p] = (err(got['tob'][p], ref['tob'][p]), TOB_REL * tmax)
    fig['en'] = (err(got['en'], ref['en']), EN_DB)
    fig['dseg'] = (err(got['dseg'], ref['dseg']), DSEG_ABS)
    r32 = np.float32(ref['raw'])
    fig['raw'] = (0.0 if np.isnan(r32) else abs(float(raw[b]) - float(r32)), RAW_REL * abs(float(r32)) + RAW_ABS if not np.isnan(r32) else 0.0)
    print('%s: nkept %d raw %r (oracle %r) ' % (tag, ref['nkept'], float(raw[b]), float(r32)) +
          ' '.join('%s %.3g/%.3g' % (k, e, bd) for k, (e, bd) in fig.items()))
    for k in ('xr', 'en', 'tob', 'dseg'):
        assert same_nan(got[k], ref[k]), (tag, k)
        assert np.isfinite(got[k][~np.isnan(ref[k])]).all(), (tag, k)
    assert bool(np.isnan(raw[b])) == bool(np.isnan(r32)), (tag, float(raw[b]), float(r32))
    for k, (e, bd) in fig.items():
        assert e <= bd, (tag, k, e, bd)
    return fig


@pytest.mark.parametrize('name', sorted(C.EXPECTED))
def test_every_stage_of_a_single_utterance(mt, name):
    """One utterance per call (B = 1, no lengths): block tails of the resampler, the single frame, 29 against 30 frames, and kept frames
    that are not contiguous across the compaction scan's 256-frame chunk."""
    x, y = C.case(name)
    raw, st = mt.estoi_stages(x.copy(), y.copy())
    compare(name, x, y, raw, st, 0, C.reference(name))
    if C.EXPECTED[name][3] < 30:
        assert raw[0] == np.float32(1e-5)


@pytest.fixture(scope='module')
def ragged_run(mt):
    X, Y, lengths, _rows = C.ragged()
    return mt.estoi_stages(X.copy(), Y.copy(), lengths=torch.from_numpy(lengths.copy()))


def test_every_stage_of_every_row_of_a_ragged_batch(ragged_run):
    """Seven rows in one padded call (lengths 6349, 6347, 2049, 6349 of digital silence, 409, 100, 0; the six lengths the case asks for
    plus the silent row), NaN behind every row's end in x and y.  Every stage of every row equals the oracle on the cut row: a read
    past a row's end, or a silent neighbour's NaN, would show as NaN in a stage.  A length of 0 is accepted by the wrapper."""
    raw, st = ragged_run
    _X, _Y, lengths, rows = C.ragged()
    refs = C.ragged_reference()
    for b, (x, y) in enumerate(rows):
        compare('ragged[%d] len %d' % (b, lengths[b]), x, y, raw, st, b, refs[b])
    assert np.isnan(raw[3]) and list(st['nkept']) == [30, 29, 9, 30, 1, 0, 0]
    assert raw[5] == raw[6] == np.float32(1e-5) and st['nkept'][5] == st['nkept'][6] == 0


def test_rows_of_a_ragged_batch_score_as_they_do_alone(mt, ragged_run):
    """Bit-identical scores: each row scored in a call of its own (at its own length; the rows of 100 and 0 samples, which the entry
    point refuses as a padded length, alone in the smallest padded buffer it accepts)."""
    raw, _st = ragged_run
    _X, _Y, lengths, rows = C.ragged()
    for b, (x, y) in enumerate(rows):
        if lengths[b] >= 409:
            alone, _ = mt.batch_estoi(x.copy(), y.copy())
        else:
            pad = np.full((1, 409), np.nan, dtype=np.float32)
            px, py = pad.copy(), pad.copy()
            px[0, :len(x)], py[0, :len(y)] = x, y
            alone, _ = mt.batch_estoi(px, py, lengths=[int(lengths[b])])
        alone = alone.cpu().numpy()
        print(b, int(lengths[b]), float(raw[b]), float(alone[0]))
        assert alone[:1].view(np.uint32)[0] == raw[b:b + 1].view(np.uint32)[0], (b, float(raw[b]), float(alone[0]))


def test_too_short_padded_length_is_refused(mt):
    """The wrapper refuses a PADDED length without a single frame (L < 409); rows that short inside a longer batch score 1e-5 (above)."""
    x, y = C.noise_pair(408, 3)
    with pytest.raises(mt._lib.NeleError):
        mt.batch_estoi(x, y)
