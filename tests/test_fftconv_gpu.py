"""GPU: nele_fir_fft_var (partitioned FFT convolution, csrc/fftconv.hip) against scipy.signal.lfilter and against the direct kernel.
Bound: 1e-12 max|ref|, what test_eval_gpu.py holds nele_fir_filter to (a float64 numpy overlap-save of the same structure stays
below 8e-16 on these cases)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

CASES = [(5000, 1), (5000, 700), (2500, 4000), (24000, 3000), (64000, 16000), (63871, 9001)]


@pytest.fixture(scope='module')
def room():
    assert torch.cuda.is_available()
    from nele_gan_amd import room
    return room


def _case(L, Lh, rows=3):
    rng = np.random.default_rng(L + Lh)
    x = rng.standard_normal((rows, L)).astype(np.float32)
    h = rng.standard_normal(Lh) * np.exp(-np.arange(Lh) / 300.0)
    return x, h


@pytest.mark.parametrize('L,Lh', CASES)
def test_fir_fft_is_scipy_lfilter(room, L, Lh):
    from scipy.signal import lfilter
    x, h = _case(L, Lh)
    y = room.fir_fft(torch.from_numpy(x).cuda(), room.prepare_bank([h])).cpu().numpy()
    ref = lfilter(h, [1], x.astype(np.float64), axis=1)
    err, bound = np.abs(y - ref).max(), 1e-12 * np.abs(ref).max()
    print('L=%d Lh=%d: max|y - scipy| = %.3e (bound %.3e)' % (L, Lh, err, bound))
    assert y.dtype == np.float64 and err <= bound


@pytest.mark.parametrize('L,Lh', CASES)
def test_fir_fft_agrees_with_the_direct_kernel(room, L, Lh):
    from nele_gan_amd import eval_metrics
    x, h = _case(L, Lh)
    xd = torch.from_numpy(x).cuda()
    y = room.fir_fft(xd, room.prepare_bank([h])).cpu().numpy()
    ref = eval_metrics.lfilter_fir(h, xd).cpu().numpy()
    err, bound = np.abs(y - ref).max(), 1e-12 * np.abs(ref).max()
    print('L=%d Lh=%d: max|y - nele_fir_filter| = %.3e (bound %.3e)' % (L, Lh, err, bound))
    assert err <= bound


def test_mixed_batch_rows_are_their_own(room):
    """three RIRs of different tap counts, four lengths: every row = its single-row call = itself inside B = 50 and B = 256, bit for
    bit, whatever the other rows and their RIRs are; exact zeros behind each row's length; the input is not read there"""
    from scipy.signal import lfilter
    rng = np.random.default_rng(11)
    hs = [rng.standard_normal(n) * np.exp(-np.arange(n) / 300.0) for n in (1, 700, 4000)]
    bank = room.prepare_bank(hs)
    lens = [5000, 2500, 4097, 256]
    Lmax = 5000
    idx = [2, 0, 1, 2, 1, 0, 2, 1]
    ln = [lens[k % 4] for k in range(8)]
    x = rng.standard_normal((8, Lmax)).astype(np.float32)
    for b in range(8):
        x[b, ln[b]:] = np.nan                                        # never read: a NaN would spread over the row's last blocks
    xd = torch.from_numpy(x).cuda()
    y = room.fir_fft(xd, bank, idx, ln).cpu().numpy()
    for b in range(8):
        ref = lfilter(hs[idx[b]], [1], x[b, :ln[b]].astype(np.float64))
        assert np.abs(y[b, :ln[b]] - ref).max() <= 1e-12 * np.abs(ref).max()
        assert not y[b, ln[b]:].any() and not np.signbit(y[b, ln[b]:]).any()
        alone = room.fir_fft(xd[b:b + 1].clone(), bank, [idx[b]], [ln[b]]).cpu().numpy()[0]
        assert np.array_equal(alone, y[b])
        short = room.fir_fft(xd[b:b + 1, :ln[b]].clone(), room.prepare_bank([hs[idx[b]]])).cpu().numpy()[0]   # own bank, own Lmax
        assert np.array_equal(short, y[b, :ln[b]])
    for B in (50, 256):
        xb = rng.standard_normal((B, Lmax)).astype(np.float32)
        ib, lb = rng.integers(0, 3, B).astype(np.int32), rng.integers(1, Lmax + 1, B).astype(np.int32)
        at = [3, B // 2, B - 8]
        for k, pos in enumerate(at):
            for r in range(4):
                xb[pos + r] = x[k * 4 % 8 + r]
                ib[pos + r], lb[pos + r] = idx[k * 4 % 8 + r], ln[k * 4 % 8 + r]
        xb_nan = np.where(np.arange(Lmax)[None, :] < lb[:, None], np.nan_to_num(xb), np.nan).astype(np.float32)
        yb = room.fir_fft(torch.from_numpy(xb_nan).cuda(), bank, ib, lb).cpu().numpy()
        assert np.isfinite(yb).all()
        for k, pos in enumerate(at):
            for r in range(4):
                assert np.array_equal(yb[pos + r], y[k * 4 % 8 + r]), (B, pos, r)


def test_rows_outside_the_bank_are_zero(room):
    x, h = _case(3000, 300, rows=4)
    y = room.fir_fft(torch.from_numpy(x).cuda(), room.prepare_bank([h]), [0, -1, 1, 0]).cpu().numpy()
    assert y[0].any() and np.array_equal(y[0] != 0, y[3] != 0) and not y[1].any() and not y[2].any()


def test_norm_clip_var_is_norm_clip_per_row(room):
    """equal lengths and no shifts: the values of nele_norm_clip; with them: the row cut, normalised, clipped and shifted on its own"""
    from nele_gan_amd import eval_metrics
    from oracle import evalpath
    rng = np.random.default_rng(9)
    a = rng.standard_normal((4, 9000))
    a[1] *= 0.01
    a[2, 100] = 40.0
    a[3] *= 3.0
    ad = torch.from_numpy(a).cuda()
    np.testing.assert_allclose(room.norm_clip_var(ad, target_rms=0.25).cpu().numpy(), eval_metrics.norm_clip(ad, target_rms=0.25).cpu().numpy(),
                               rtol=1e-6, atol=1e-9)
    ln, sh = np.asarray([9000, 4000, 8999, 513], np.int32), np.asarray([0, 37, 5, 512], np.int32)
    i32 = lambda v: torch.from_numpy(v).cuda()
    out = room.norm_clip_var(ad, lengths=i32(ln), out_shift=i32(sh), target_rms=0.25, keep64=True).cpu().numpy()
    add = rng.standard_normal((4, 9000)).astype(np.float32)
    mix = room.norm_clip_var(torch.from_numpy(out).cuda(), add=torch.from_numpy(add).cuda(), lengths=i32(ln - sh), add_shift=i32(sh)).cpu().numpy()
    for b in range(4):
        v = a[b, :ln[b]]
        ref = evalpath.clip(v / evalpath.rms(v) * 0.25)[sh[b]:]
        np.testing.assert_allclose(out[b, :len(ref)], ref, rtol=1e-12, atol=1e-15)
        assert not out[b, len(ref):].any()
        ref2 = evalpath.clip(ref + add[b, sh[b]:ln[b]])
        np.testing.assert_allclose(mix[b, :len(ref2)], ref2.astype(np.float32), rtol=1e-6, atol=1e-9)
        assert not mix[b, len(ref2):].any()
