"""GPU: the order and the cache policy of the memory operations in the envelope-rate kernels of csrc/haspi.hip.  In its gain
instantiation, each 16-sample group of haspi_bank_scan_kernel requests the NEXT group's inputs (the middle-ear samples and the control
envelope) behind their last use and ahead of its own stores; the last group of a chunk requests itself again.  The envelopes are stored
and loaded with the nontemporal hint.  What that can break is an address or an ordering, never the arithmetic: a request that reaches
into the next chunk, the next row or behind the row's padded end, a group that runs on the values of the wrong group, a load that
passes the store it depends on.

One ragged batch at 16 kHz (n24 = 1.5 L, scan chunks of GS_LC = 1536 samples, groups of GS_RC = 16), a row for each such seam:
  L =  800   n24 =  1200          shorter than one chunk
  L = 2048   n24 =  3072          exactly two chunks: the last group of the row ends on the chunk's end
  L = 4118   n24 =  6177          16 x 386 + 1: a fifth chunk of three groups whose last group holds ONE sample
  L = 2800   n24 =  4200          three chunks: the second half-wave of the last pair has no chunk
  L = 8000   n24 = 12000          an ordinary 0.5 s row (the padded length)
x and y hold NaN behind every row's end.

(a) every stage buffer of every row is bit-identical to the same utterance run alone (B = 1; padded to its own length, or to the 2400
    samples that a call accepts at least) and at another position of the batch (the rows in reverse order);
(b) the same batch gives identical bits in a workspace that a longer and larger batch used just before (haspi_stages itself fills a new
    workspace with 0xFF): prefetched values from behind a row's end would differ between the two;
(c) every stage of every row is within the bounds of test_haspi_stages_gpu.py / haspi_cases.py against the float64 oracle."""
import numpy as np
import pytest

import haspi_cases as C
import test_haspi_stages_gpu as S

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

FS = 16000
LENGTHS = (800, 2048, 4118, 2800, 8000)
MIN_L = 2400                                              # nele_metric_haspi_var: the shortest padded length of a call
STAGES = ('r24', 'rinfo', 'mid', 'ctl', 'bw', 'shift', 'env', 'lp', 'index', 'act', 'cep', 'cmean', 'xf', 'cm', 'info')


def test_the_rows_sit_on_the_seams_they_are_named_for():
    n24 = [C.dims(L, FS)[0] for L in LENGTHS]
    assert n24 == [1200, 3072, 6177, 4200, 12000]
    assert n24[0] < C.GS_LC and n24[1] == 2 * C.GS_LC and n24[2] == C.GS_RC * 386 + 1 and n24[2] > 4 * C.GS_LC
    assert -(-n24[3] // C.GS_LC) == 3 and -(-n24[2] // C.GS_LC) == 5


@pytest.fixture(scope='module')
def mt():
    assert torch.cuda.is_available()
    from nele_gan_amd import metrics
    return metrics


@pytest.fixture(scope='module')
def rows():
    return [C.am_pair(L, FS, 7000 + L) for L in LENGTHS]


def padded(rows, order, Lmin=0):
    Lmax = max([Lmin] + [len(rows[r][0]) for r in order])
    X = np.full((len(order), Lmax), np.nan, dtype=np.float32)
    Y = X.copy()
    for b, r in enumerate(order):
        x, y = rows[r]
        X[b, :len(x)], Y[b, :len(y)] = x, y
    return X, Y, np.array([len(rows[r][0]) for r in order], dtype=np.int32)


@pytest.fixture(scope='module')
def batch_run(mt, rows):
    X, Y, lengths = padded(rows, range(len(rows)))
    return S.run(mt, X, Y, FS, lengths=lengths)


def same_bits(tag, raw_a, st_a, a, raw_b, st_b, b):
    assert raw_a[a:a + 1].view(np.uint32)[0] == raw_b[b:b + 1].view(np.uint32)[0], (tag, 'raw', float(raw_a[a]), float(raw_b[b]))
    for k in STAGES:
        u, v = np.ascontiguousarray(st_a[k][a]), np.ascontiguousarray(st_b[k][b])
        assert u.shape == v.shape and u.dtype == v.dtype, (tag, k, u.shape, v.shape)
        assert u.tobytes() == v.tobytes(), (tag, k, 'first difference at', int(np.flatnonzero(u.view(np.uint8).ravel() != v.view(np.uint8).ravel())[0]))


def test_a_row_has_the_bits_of_the_utterance_alone_and_at_another_position(mt, rows, batch_run):
    raw, _info, st = batch_run
    order = list(range(len(rows)))[::-1]
    X, Y, lengths = padded(rows, order)
    raw_r, _i, st_r = S.run(mt, X, Y, FS, lengths=lengths)
    for b, r in enumerate(order):
        same_bits('row %d at position %d' % (r, b), raw, st, r, raw_r, st_r, b)
    for r in range(len(rows)):
        X, Y, lengths = padded(rows, [r], Lmin=MIN_L)
        raw_1, _i, st_1 = S.run(mt, X, Y, FS, lengths=lengths)
        same_bits('row %d alone' % r, raw, st, r, raw_1, st_1, 0)


def stages_in(mt, ws, X, Y, lengths):
    """The per-sample buffers and the envelope frames of one call in the workspace ws as it stands (metrics.haspi_stages fills a new one
    with 0xFF), cut to every row's own extent as haspi_stages cuts them -> (raw, {name: [rows]})"""
    from nele_gan_amd import _lib
    from nele_gan_amd._lib import c_longlong, call, ptr, stream
    x, y, _ = mt._pair(X, Y)
    B, L = x.shape
    nsub = _lib.lib.nele_metric_haspi_nsub(L, FS)
    assert ws.numel() >= _lib.lib.nele_metric_haspi_workspace_bytes(B, L, FS)
    raw = torch.empty(B, device=x.device)
    info = torch.full((B, 2), -1, dtype=torch.int32, device=x.device)
    call('nele_metric_haspi_var_hl', ptr(x), ptr(y), ptr(mt._lens(lengths, x.device)), B, L, FS, None, None, 0, ptr(ws), ws.numel(), ptr(raw), None,
         ptr(info), 0, stream())
    buf = (c_longlong * 45)()
    assert _lib.lib.nele_metric_haspi_sections(B, L, FS, buf, 15) == 15
    sec = [(int(buf[3 * k]), int(buf[3 * k + 1]), int(buf[3 * k + 2])) for k in range(15)]
    r24, mid, _bw, shift, _rinfo, env, ctl, lp = mt._section_rows(ws, sec[:8], B)
    out = {k: [] for k in ('r24', 'mid', 'ctl', 'env', 'lp')}
    for b in range(B):
        n24 = C.dims(int(lengths[b]), FS)[0]
        ns = -(-n24 // 9)
        out['r24'].append(r24[b].view(np.float32).reshape(2, -1)[:, :n24].copy())
        out['mid'].append(mid[b].view(np.float64).reshape(2, -1)[:, :n24].copy())
        out['ctl'].append(ctl[b].view(np.float32).reshape(2, -1, 32)[:, :n24].copy())
        out['env'].append(env[b].view(np.float32).reshape(2, -1, 32)[:, :n24].copy())
        sh = shift[b].view(np.int32)
        di = (((26 - sh) % 9 + 9) % 9 + sh - 26) // 9                      # group-space rows -> frame order, as in haspi_stages
        g = np.arange(ns)[:, None] - di[None, :]
        fr = lp[b].view(np.float64).reshape(2, nsub + 4, 32)[:, np.clip(g, 0, nsub + 3), np.arange(32)[None, :]]
        out['lp'].append(np.where((g >= 0)[None], fr, 0.0))
    return raw.cpu().numpy(), info.cpu().numpy(), out


def test_a_workspace_used_by_a_longer_batch_gives_the_same_bits(mt, rows):
    from nele_gan_amd import _lib
    X, Y, lengths = padded(rows, range(len(rows)))
    B, L = X.shape
    Lbig = 11000                                                          # other row strides, chunk counts and section offsets
    xb, yb = C.am_pair(Lbig, FS, 4242)
    XB, YB = np.tile(xb, (B + 2, 1)), np.tile(yb, (B + 2, 1))
    nbig = int(_lib.lib.nele_metric_haspi_workspace_bytes(B + 2, Lbig, FS))
    assert nbig > int(_lib.lib.nele_metric_haspi_workspace_bytes(B, L, FS))
    ws = torch.full((nbig,), 255, dtype=torch.uint8, device='cuda')
    raw0, info0, st0 = stages_in(mt, ws, X, Y, lengths)                    # clean: nothing but 0xFF where no kernel wrote
    stages_in(mt, ws, XB, YB, np.full(B + 2, Lbig, dtype=np.int32))
    raw1, info1, st1 = stages_in(mt, ws, X, Y, lengths)                    # the same workspace, now full of the longer batch's values
    assert np.array_equal(info0, info1) and (info0[:, 1] == 0).all(), (info0.tolist(), info1.tolist())
    assert raw0.tobytes() == raw1.tobytes(), (raw0.tolist(), raw1.tolist())
    for k, per_row in st0.items():
        for b, a in enumerate(per_row):
            assert np.isfinite(a).all(), (k, b)
            assert a.tobytes() == st1[k][b].tobytes(), (k, b, float(np.max(np.abs(a - st1[k][b]))))


def test_every_stage_of_every_row_is_within_the_oracle_bounds(rows, batch_run):
    raw, info, st = batch_run
    for b, (x, y) in enumerate(rows):
        pure = C.oracle_stages(x, y, FS)
        S.compare('order[%d] len %d' % (b, len(x)), x, y, FS, raw, info, st, b, S.references(pure, st['r24'][b], x, y, FS, None, None))
