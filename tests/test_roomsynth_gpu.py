"""GPU: nele_rir_synth (csrc/roomsynth.hip) against tests/roomsynth_ref.py - the float64 restatement of DESIGN.md section 13 - and the
synthesised bank through the room path that --rir feeds.

Bound per tap: |h_gpu[n] - h_ref[n]| <= 1e-10 SA[n], SA[n] = sum of |A| over the images that reach tap n.  The delay carries about
tau eps64 (4e-12 at 16 000 taps) and the sinc's slope is below pi, so a term is off by about 1e-11 A at worst; a wrong image, parity or
wall costs 1e-2.  Taps no image reaches must be exact zeros.
Lengths: around the kernel's tile T (1, 37, T - 1, T, T + 1, 2 T + 40), and one batch of rows with different taps up to 4000 - 86 m,
where a tile's shell holds some 20 000 images: several pair batches, chunks that overflow, both z intervals of a pair.
Measured on an MI355X: largest ratio 6.57e-14 (six_betas, 4000 taps); the calibrated bank of four 0.3 to 4.3 % from its targets (bound 5 %);
the exported folder moves Room.apply's rows by at most 2.6e-4 of their norm."""
import os

import numpy as np
import pytest

import roomsynth_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

SENTINEL = -7.25


def _room(L, s, m, beta):
    return np.concatenate([np.asarray(L, float), np.asarray(s, float), np.asarray(m, float), np.broadcast_to(np.asarray(beta, float), (6,))])


BASE = ((3.1, 4.2, 2.6), (0.9, 1.7, 1.2), (2.3, 3.1, 1.5))
ROOMS = {
    'six_betas': _room(*BASE, [0.8, 0.72, 0.8, 0.76, 0.64, 0.8]),
    'flat': _room((9.5, 3.2, 2.4), (2.1, 1.3, 1.1), (7.3, 2.2, 1.4), [0.7, 0.75, 0.8, 0.6, 0.85, 0.65]),
    'absorbing': _room(*BASE, 0.0),
    'one_dead_wall': _room(*BASE, [0.0, 0.9, 0.8, 0.8, 0.8, 0.8]),
    'beta_one_axis': _room(*BASE, [0.7, 0.7, 1.0, 1.0, 0.6, 0.6]),
    'close': _room((3.1, 4.2, 2.6), (1.5, 2.0, 1.3), (1.5 + 0.12, 2.0 + 0.16, 1.3), [0.8, 0.72, 0.8, 0.76, 0.64, 0.8]),       # 0.2 m apart
    'near_wall': _room((3.1, 4.2, 2.6), (0.31, 1.7, 1.2), (2.3, 3.1, 1.5), [0.8, 0.72, 0.8, 0.76, 0.64, 0.8]),
}
NAMES = list(ROOMS)
MIXED_TAPS = {'six_betas': 4000, 'flat': 3000, 'absorbing': 600, 'one_dead_wall': 700, 'beta_one_axis': 1500, 'close': 300, 'near_wall': 257}
_REF = {}


def _ref(name, taps):
    """(h, SA) of the room's first ``taps`` taps: computed once at the longest length any test asks for (a tap's sum does not depend on taps)"""
    from nele_gan_amd import roomsynth
    longest = max(MIXED_TAPS[name], 2 * roomsynth.TILE + 40)
    if name not in _REF:
        _REF[name] = R.rir(ROOMS[name], longest)
    h, SA = _REF[name]
    return h[:taps], SA[:taps]


def _raw(rooms, taps, N):
    """nele_rir_synth into a sentinel-filled [R + 1][N] buffer -> (out [R + 1, N], status [R]) on the host"""
    from nele_gan_amd import _lib, roomsynth
    roomsynth.library()                                      # declares the entry point's signature
    R_ = len(rooms)
    packed = np.zeros((R_, 16))
    packed[:, :15] = np.stack(rooms)
    d_rooms = torch.from_numpy(packed).cuda()
    d_taps = torch.from_numpy(np.asarray(taps, dtype=np.int32)).cuda()
    out = torch.full((R_ + 1, N), SENTINEL, dtype=torch.float64, device='cuda')
    status = torch.full((R_,), -1, dtype=torch.int32, device='cuda')
    _lib.call('nele_rir_synth', _lib.ptr(d_rooms), _lib.ptr(d_taps), R_, N, 16000.0, 343.0, 40, _lib.ptr(out), _lib.ptr(status), None, _lib.stream())
    torch.cuda.synchronize()
    return out.cpu().numpy(), status.cpu().numpy()


def _check_rows(out, status, names, taps, N):
    worst = 0.0
    for r, (name, t) in enumerate(zip(names, taps)):
        h, SA = _ref(name, t)
        assert status[r] == 0, (name, status[r])
        err = np.abs(out[r, :t] - h)
        reached = SA > 0
        ratio = float((err[reached] / SA[reached]).max()) if reached.any() else 0.0
        worst = max(worst, ratio)
        print('%s taps %d: max |h_gpu - h_ref| / SA = %.3g (%d of %d taps reached)' % (name, t, ratio, int(reached.sum()), t))
        assert (err <= 1e-10 * SA).all(), (name, t, ratio)
        assert not out[r, t:].any(), name                    # exact zeros behind taps[r]
    assert (out[len(names)] == SENTINEL).all()               # the guard row behind the output
    return worst


def _lengths():
    from nele_gan_amd import roomsynth
    T = roomsynth.TILE
    return (1, 37, T - 1, T, T + 1, 2 * T + 40)


@pytest.mark.parametrize('k', range(6))
def test_kernel_against_the_reference_at_each_length(k):
    N = _lengths()[k]
    out, status = _raw([ROOMS[n] for n in NAMES], [N] * len(NAMES), N)
    _check_rows(out, status, NAMES, [N] * len(NAMES), N)


def test_kernel_against_the_reference_rows_with_different_taps():
    taps = [MIXED_TAPS[n] for n in NAMES]
    N = max(taps) + 100                                      # columns behind the longest row: zeros too
    out, status = _raw([ROOMS[n] for n in NAMES], taps, N)
    worst = _check_rows(out, status, NAMES, taps, N)
    print('largest ratio over the batch: %.3g' % worst)
    assert np.abs(out[0, 3000:4000]).max() > 0              # the late taps hold a response


def test_a_rooms_bits_are_its_own():
    from nele_gan_amd import roomsynth
    N = 2 * roomsynth.TILE + 40
    room = ROOMS['six_betas']
    alone, st = roomsynth.synth_rirs(room[None, :], N)
    assert int(st[0]) == 0 and float(alone.abs().max()) > 0
    others = [ROOMS[n] for n in ('flat', 'absorbing', 'one_dead_wall', 'beta_one_axis', 'close', 'near_wall')]
    batch = [room, others[0], others[1], room, others[2], others[3], room]
    taps = [N, 300, N, N, 37, N, N]
    for run in range(2):
        h, st = roomsynth.synth_rirs(np.stack(batch), taps)
        for pos in (0, 3, 6):
            assert torch.equal(h[pos], alone[0]), (run, pos)
    # a longer row of the same room: the same bits where both have taps
    longer, _ = roomsynth.synth_rirs(room[None, :], 1500)
    assert torch.equal(longer[0, :N], alone[0])
    # at 1290 taps the room's last tile (from tap 1280) walks 247 pairs and takes its powers from pow(); as a whole tile of the 1500-tap
    # row it walks 336 and builds the power tables: the same bits
    short, _ = roomsynth.synth_rirs(room[None, :], 1290)
    assert torch.equal(longer[0, :1290], short[0])


def test_status_bits_and_zero_rows():
    from nele_gan_amd import roomsynth
    good = ROOMS['six_betas']
    bad_size, bad_pos, bad_close, bad_beta, bad_nan = (good.copy() for _ in range(5))
    bad_size[1] = 0.0
    bad_pos[3] = 3.1                                         # the source on the wall
    bad_close[6:9] = bad_close[3:6] + np.asarray([0.005, 0.0, 0.0])
    bad_beta[11] = 1.0001
    bad_nan[0] = np.nan
    bad_nan[14] = -0.1
    N = roomsynth.TILE + 1
    out, status = _raw([bad_size, good, bad_pos, bad_close, bad_beta, bad_nan], [N] * 6, N + 3)
    assert status.tolist() == [roomsynth.BAD_SIZE, 0, roomsynth.BAD_POSITION, roomsynth.BAD_POSITION, roomsynth.BAD_BETA,
                               roomsynth.BAD_SIZE | roomsynth.BAD_BETA]
    for r in (0, 2, 3, 4, 5):
        assert not out[r].any(), r
    alone, _ = roomsynth.synth_rirs(good[None, :], N)
    assert np.array_equal(out[1, :N], alone[0].cpu().numpy()) and not out[1, N:].any()
    assert (out[6] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------------------ bank and plumbing
_BANK = {}


def _bank():
    from nele_gan_amd import roomsynth
    if 'b' not in _BANK:
        _BANK['b'] = roomsynth.synth_bank(4, seed=21, t60_s=(0.15, 0.25))
    return _BANK['b']


def test_calibration_and_t60_on_the_device():
    from nele_gan_amd import roomsynth
    bank = _bank()
    assert bank.names == ['synth%04d' % i for i in range(4)] and len(bank.rooms) == 4
    for rec, h in zip(bank.rooms, bank.rirs):
        print('%s: target %.4f s, measured %.4f s, %d taps' % (rec['name'], rec['t60_target'], rec['t60_measured'], rec['taps']))
        assert 0.15 <= rec['t60_target'] <= 0.25 and len(h) == rec['taps'] == int(np.ceil(rec['t60_target'] * 16000))
        assert abs(rec['t60_measured'] / rec['t60_target'] - 1.0) <= 0.05
        assert all(0.0 < b < 1.0 for pair in rec['beta'] for b in pair)
    # t60_of on the device against the reference's, on a response of the kernel
    h, _ = roomsynth.synth_rirs([roomsynth.room_row(list(bank.rooms[0]['L']) + list(bank.rooms[0]['s']) + list(bank.rooms[0]['m'])
                                                    + [b for p in bank.rooms[0]['beta'] for b in p])], bank.rooms[0]['taps'])
    assert float(roomsynth.t60_of(h[0], 16000)) == pytest.approx(R.t60(h[0].cpu().numpy()), rel=1e-9)
    assert float(roomsynth.t60_of(h, 16000)[0]) == pytest.approx(bank.rooms[0]['t60_measured'], rel=1e-9)
    again = roomsynth.synth_bank(4, seed=21, t60_s=(0.15, 0.25))
    assert again.sample_hash() == bank.sample_hash() and again.record() == bank.record()


def _apply_batch(B=4, L=4096):
    from nele_gan_amd import synth
    c, v = synth.batch(B, L, start=70)
    return c, (c * np.float32(2.0)).copy(), v


IDS = np.asarray([0, 3, -1, 1], np.int32)


def test_room_apply_with_the_synthesised_bank_against_the_oracle():
    from nele_gan_amd import room
    from oracle import evalpath
    bank = _bank()
    c, enh, v = _apply_batch()
    clean_a, mixed, la = room.Room(bank).apply(torch.from_numpy(c).cuda(), torch.from_numpy(enh).cuda(), torch.from_numpy(v).cuda(), IDS)
    clean_a, mixed, la = clean_a.cpu().numpy(), mixed.cpu().numpy(), la.cpu().numpy()
    for b in range(4):
        rir = None if IDS[b] < 0 else bank.rirs[IDS[b]]
        assert rir is None or rir.dtype == np.float32
        ca, mx = evalpath.listening_condition(c[b], enh[b], v[b], rir, enh_rms=0.0)
        assert la[b] == len(ca) == len(mx)
        np.testing.assert_allclose(clean_a[b, :la[b]], ca, rtol=1e-5, atol=2e-8)
        np.testing.assert_allclose(mixed[b, :la[b]], mx, rtol=1e-5, atol=2e-8)
        assert not clean_a[b, la[b]:].any() and not mixed[b, la[b]:].any()


def test_canonical_step_in_synthesised_rooms():
    from nele_gan_amd import synth
    from nele_gan_amd.train_nele import GanTrainer
    bank = _bank()
    c, v = synth.batch(4, 16384, start=70)
    tr = GanTrainer('siib&estoi', room=bank)
    _, _, tgt = tr.canonical_step(torch.from_numpy(c).cuda(), torch.from_numpy(v).cuda(), rir_ids=IDS)
    assert bool(torch.isfinite(tgt).all())
    st = tr.check_status()
    assert not any(st[k] for k in ('siib_undefined', 'haspi_below_threshold', 'skipped_g_steps', 'skipped_d_steps'))
    assert bank.ids(['a.wav', 'b.wav', 'a.wav']).tolist()[0] == bank.ids(['/elsewhere/a.wav']).tolist()[0]


def test_exported_folder_reads_back_within_pcm16_reach(tmp_path):
    """A file holds rint(32767 scale h) / 32768: against scale' h, scale' = scale 32767 / 32768, every tap is off by at most
    q = 0.504 / 32768 - half a quantisation step of the file, whose peak 0.9 is step 29 490 of 32 767, and the float32 rounding of
    the writer's product.  Filtering x with h + e, |e_k| <= q / scale' over T taps, moves y = h * x by at most ||e||_1 ||x||_2 <=
    T q / scale' ||x||_2 in the 2-norm (Young), and scaling both to the same rms at most doubles the relative difference: the rows of
    Room.apply differ by at most 2 T (q / scale') ||x||_2 / ||y||_2 of their norm (+ 1e-5 for their float32 values)."""
    from scipy.signal import lfilter
    from nele_gan_amd import room, roomsynth
    bank = _bank()
    out_dir = str(tmp_path / 'rooms')
    listed = roomsynth.export_bank(bank, out_dir)
    assert sorted(os.listdir(out_dir)) == ['rooms.json'] + [n + '.wav' for n in bank.names]
    back = room.RirBank(out_dir)
    assert back.names == bank.names
    q = 0.504 / 32768.0                                     # the writer's float32 product 32767 x is itself off by up to 2 * 29490 * 2^-24 = 0.0035 steps
    for rec, h, hf in zip(listed, bank.rirs, back.rirs):
        scale = rec['scale'] * 32767.0 / 32768.0
        assert len(hf) == len(h) and float(np.abs(hf).max()) == pytest.approx(0.9 * 32767.0 / 32768.0, abs=2 * q)
        assert np.abs(hf.astype(np.float64) - scale * h.astype(np.float64)).max() <= q
    c, enh, v = _apply_batch()
    args = [torch.from_numpy(t).cuda() for t in (c, enh, v)]
    ca0, mx0, la0 = room.Room(bank).apply(*args, IDS)
    ca1, mx1, la1 = room.Room(back).apply(*args, IDS)
    assert torch.equal(la0, la1)
    for b in range(4):
        if IDS[b] < 0:
            assert torch.equal(ca0[b], ca1[b]) and torch.equal(mx0[b], mx1[b])
            continue
        rec, h = listed[IDS[b]], bank.rirs[IDS[b]].astype(np.float64)
        e_per_tap = q / (rec['scale'] * 32767.0 / 32768.0)
        n = int(la0[b])
        shift = bank.b[IDS[b]]
        for got0, got1, x, taps, added in ((mx0, mx1, enh[b], len(h), v[b, shift:shift + n]), (ca0, ca1, c[b], shift + bank.tau, None)):
            y = lfilter(h[:taps], [1.0], x.astype(np.float64))
            bound = 2.0 * taps * e_per_tap * np.linalg.norm(x) / np.linalg.norm(y) + 1e-5
            # the norm the difference is measured against is the row's own: of the n samples Room.apply keeps of the filtered, scaled row -
            # for `mixed` after taking the noise off again (mixed = that row + the SAME shifted noise, so its difference is the row's)
            row0 = got0[b, :n].double().cpu().numpy() - (0.0 if added is None else added.astype(np.float64))
            ref_norm = float(np.linalg.norm(row0))
            assert 0.8 * 0.03 * np.sqrt(n) <= ref_norm <= 1.2 * 0.03 * np.sqrt(n)       # rms 0.03: nothing was clipped, the noise came off
            diff = float(torch.linalg.vector_norm((got0[b, :n] - got1[b, :n]).double()))
            print('row %d, %d taps: difference %.3g of the row norm (bound %.3g)' % (b, taps, diff / ref_norm, bound))
            assert diff <= bound * ref_norm
