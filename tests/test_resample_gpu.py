"""GPU: the polyphase resampler (csrc/resample.hip, nele_gan_amd/resample.py) against scipy.signal.resample_poly with the library's own
taps, on the smallest shapes at which the kernel can go wrong - rows shorter than the filter, output lengths around the kernel's tile,
several tiles, the index that passes 2^31 - then what does not depend on the batch, closed forms, mixed rates, the command line and
the loaders' opt-in switches.

Bound per sample (resample_ref.bound): |y - float32(y64)| <= spacing(float32(|y64|)) + 1e-12 max|x|.  The first term is one float32 ulp,
for values the float64 summation order moves across a rounding boundary; the second covers zero crossings: K eps64 max|h| max|x| with a
tenfold margin, max|h| <= 1."""
import csv
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import resample_ref as R

pytestmark = pytest.mark.gpu

CASES = [(up, down, preset) for up, down in R.PAIRS for preset in sorted(R.PRESETS)]
SENTINEL = -7


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _in_len(up, down, pick):
    """the input length L whose output length ceil(L up / down) is the largest below / the smallest at or above / above the target"""
    kind, target = pick
    L = target * down // up
    while R.out_len(L, up, down) >= target:
        L -= 1
    if kind == 'below':
        return L                                             # largest L with n_out < target
    L += 1
    if kind == 'above':
        while R.out_len(L, up, down) <= target:
            L += 1
    return L


def _lengths(up, down):
    from nele_gan_amd import resample
    T = resample.TILE
    return [0, 1, 2, 37, _in_len(up, down, ('below', T)), _in_len(up, down, ('at', T)), _in_len(up, down, ('above', T)),
            _in_len(up, down, ('at', 2 * T + 40))]


_BATCHES = {}


def _batch(up, down, preset):
    """One padded batch per case, its scipy reference and the kernel's output on it - computed once, never changed."""
    from nele_gan_amd import resample
    key = (up, down, preset)
    if key in _BATCHES:
        return _BATCHES[key]
    T = resample.TILE
    zeros, beta = R.PRESETS[preset]
    lens = np.asarray(_lengths(up, down), dtype=np.int32)
    n_out = [R.out_len(int(n), up, down) for n in lens]
    assert n_out[4] < T <= n_out[5] <= n_out[6] and n_out[6] > T and 2 * T < n_out[7] <= 3 * T, n_out
    rng = _rng('test_against_scipy[%d-%d-%s]' % key)
    x = rng.standard_normal((len(lens), int(lens.max()))).astype(np.float32)     # what lies behind a row's length must count as zero
    h = resample.taps(up, down, zeros, beta)
    ref = [R.scipy_resample(x[b, :n], up, down, h) for b, n in enumerate(lens)]
    rs = resample.Resampler(16000 * down, 16000 * up, preset)
    assert (rs.up, rs.down) == (up, down)
    Lout = max(n_out) + 5
    y = torch.full((len(lens), Lout), float('nan'), dtype=torch.float32, device='cuda')
    no = torch.full((len(lens),), SENTINEL, dtype=torch.int32, device='cuda')
    xd = torch.from_numpy(x).cuda()
    rs.apply(xd, lens, out=(y, no))
    torch.cuda.synchronize()
    _BATCHES[key] = dict(x=x, xd=xd, lens=lens, n_out=n_out, ref=ref, rs=rs, y=y.cpu().numpy(), no=no.cpu().numpy(), Lout=Lout)
    return _BATCHES[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize('up,down,preset', CASES)
def test_against_scipy(up, down, preset):
    c = _batch(up, down, preset)
    assert c['no'].tolist() == c['n_out'] == [len(r) for r in c['ref']]
    worst = 0.0
    for b, n in enumerate(c['n_out']):
        row = c['y'][b]
        assert np.array_equal(_bits(row[n:]), np.zeros(c['Lout'] - n, dtype=np.int32)), 'row %d: not exact zeros behind its length' % b
        if n:
            want = c['ref'][b]
            xmax = float(np.abs(c['x'][b, :c['lens'][b]]).max())
            err = np.abs(row[:n].astype(np.float64) - want.astype(np.float32).astype(np.float64))
            tol = R.bound(want, xmax)
            worst = max(worst, float((err / tol).max()))
    print('%d/%d %s: largest error / bound %.3f' % (up, down, preset, worst))
    assert worst <= 1.0


@pytest.mark.parametrize('up,down,preset', CASES)
def test_a_rows_bits_are_its_own(up, down, preset):
    c = _batch(up, down, preset)
    rs, lens, B = c['rs'], c['lens'], len(c['lens'])
    # alone: B = 1, Lmax = the row's own length
    for b in range(B):
        n = int(lens[b])
        xa = c['xd'][b:b + 1, :max(n, 1)].contiguous()
        ya, na = rs.apply(xa, [n])
        assert int(na[0]) == c['n_out'][b] and ya.shape[1] == max(c['n_out'][b], 1)
        assert np.array_equal(_bits(ya[0].cpu().numpy()[:c['n_out'][b]]), _bits(c['y'][b, :c['n_out'][b]])), 'row %d alone' % b
    # another batch: other Lmax in and out, rows in another order
    order = np.asarray([5, 0, 7, 2, 6, 1, 4, 3])
    x2 = torch.full((B, c['x'].shape[1] + 13), 3.0, dtype=torch.float32, device='cuda')
    x2[:, :c['x'].shape[1]] = c['xd'][torch.from_numpy(order).cuda()]
    y2 = torch.full((B, c['Lout'] + 301), float('nan'), dtype=torch.float32, device='cuda')
    n2 = torch.full((B,), SENTINEL, dtype=torch.int32, device='cuda')
    rs.apply(x2, lens[order], out=(y2, n2))
    y2 = y2.cpu().numpy()
    assert n2.cpu().tolist() == [c['n_out'][b] for b in order]
    for i, b in enumerate(order):
        assert np.array_equal(_bits(y2[i, :c['Lout']]), _bits(c['y'][b])), 'row %d in another batch' % b
        assert not y2[i, c['Lout']:].any()
    # row_ids naming some rows, in reverse: the others keep their sentinels
    ids = [7, 5, 4, 2, 0]
    y3 = torch.full((B, c['Lout']), float('nan'), dtype=torch.float32, device='cuda')
    n3 = torch.full((B,), SENTINEL, dtype=torch.int32, device='cuda')
    rs.apply(c['xd'], lens, row_ids=ids, out=(y3, n3))
    y3, n3 = y3.cpu().numpy(), n3.cpu().numpy()
    for b in range(B):
        if b in ids:
            assert n3[b] == c['n_out'][b] and np.array_equal(_bits(y3[b]), _bits(c['y'][b])), 'row %d through row_ids' % b
        else:
            assert n3[b] == SENTINEL and np.isnan(y3[b]).all(), 'row %d was not named' % b


def test_64_bit_indices():
    """13 500 000 samples at 160 / 441 give 4 897 960 outputs.  The 2048 outputs around n = 4 869 615 (the figure the feature's issue
    names) hold both crossings of 2^31: n * 441 at n = 4 869 578 and c = n * 441 + half at n = 4 869 546."""
    from nele_gan_amd import resample
    up, down, L = 160, 441, 13500000
    cross = 4869615
    half = R.half_width(up, down, R.PRESETS['high'][0])
    assert cross - 1024 <= -(-(2 ** 31 - half) // down) == 4869546 and -(-2 ** 31 // down) == 4869578 < cross + 1024
    x = _rng('test_64_bit_indices').standard_normal(L).astype(np.float32)
    rs = resample.Resampler(44100, 16000, 'high')
    y, n = rs.apply(torch.from_numpy(x).cuda().unsqueeze(0), [L])
    assert int(n[0]) == 4897960 == y.shape[1]
    y = y[0].cpu().numpy()
    h = resample.taps(up, down, *R.PRESETS['high'])
    xmax = float(np.abs(x).max())
    for name, ns in (('around the crossing', range(cross - 1024, cross + 1024)), ('the last 2048', range(4897960 - 2048, 4897960))):
        want = R.resample(x, up, down, h, outputs=ns)
        err = np.abs(y[ns.start:ns.stop].astype(np.float64) - want.astype(np.float32).astype(np.float64))
        worst = float((err / R.bound(want, xmax)).max())
        print('%s: largest error / bound %.3f' % (name, worst))
        assert worst <= 1.0, name


@pytest.mark.parametrize('sr_in', (44100, 48000, 8000, 22050))
def test_closed_forms(sr_in):
    """A unit sinusoid in the common pass band comes out as the same sinusoid sampled at 16 kHz; a tone between the new and the old
    Nyquist frequency leaves nothing.  Quality 'high', away from the first and last 72 outputs."""
    from nele_gan_amd import resample
    n_in = sr_in // 2
    t = np.arange(n_in, dtype=np.float64) / sr_in
    tones = [1000.0, 0.8 * min(sr_in, 16000) / 2]
    stop = {44100: 14332.0, 48000: 15600.0, 22050: 9600.0}.get(sr_in)
    x = np.stack([np.sin(2 * np.pi * f * t) for f in tones + ([stop] if stop else [])]).astype(np.float32)
    y, n = resample.resample(torch.from_numpy(x).cuda(), [n_in] * len(x), sr_in)
    assert n.cpu().tolist() == [8000] * len(x)
    y = y.cpu().numpy().astype(np.float64)[:, 72:8000 - 72]
    to = np.arange(72, 8000 - 72, dtype=np.float64) / 16000.0
    for k, f in enumerate(tones):
        err = float(np.abs(y[k] - np.sin(2 * np.pi * f * to)).max())
        print('%d Hz -> 16 kHz, %g Hz tone: error %.3g' % (sr_in, f, err))
        assert err <= 1e-5
    if stop:
        res = float(np.abs(y[len(tones)]).max())
        print('%d Hz -> 16 kHz, %g Hz tone: residual %.3g' % (sr_in, stop, res))
        assert res <= 1e-5


def test_mixed_rates_in_one_call():
    from nele_gan_amd import resample
    rates = [8000, 16000, 44100, 48000]
    lens = [700, 1000, 1931, 2100]
    x = _rng('test_mixed_rates_in_one_call').standard_normal((4, 2100)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    y, n = resample.resample(xd, lens, rates)
    y, n = y.cpu().numpy(), n.cpu().tolist()
    assert n == [1400, 1000, 701, 700] and y.shape == (4, 1400)
    for b, (r, L) in enumerate(zip(rates, lens)):
        y1, n1 = resample.resample(xd[b:b + 1, :L].contiguous(), [L], r)
        assert int(n1[0]) == n[b]
        assert np.array_equal(_bits(y1[0].cpu().numpy()), _bits(y[b, :n[b]])) and not y[b, n[b]:].any()
    assert np.array_equal(_bits(y[1, :1000]), _bits(x[1, :1000]))                 # the row already at 16 kHz is a copy
    assert len(set(k[0] for k in resample._CACHE)) >= 4                           # one Resampler per rate, kept


# ------------------------------------------------------------------------------------------------ files
def _write_pcm16(path, x, sr):
    body = np.clip(np.rint(np.asarray(x, dtype=np.float32) * np.float32(32767.0)), -32768, 32767).astype('<i2').tobytes()
    with open(path, 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', 36 + len(body)) + b'WAVEfmt ' + struct.pack('<IHHIIHH', 16, 1, 1, sr, sr * 2, 2, 16) + b'data'
                + struct.pack('<I', len(body)) + body)


def _write_float32(path, x, sr):
    body = np.asarray(x, dtype='<f4').tobytes()
    with open(path, 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', 36 + len(body)) + b'WAVEfmt ' + struct.pack('<IHHIIHH', 16, 3, 1, sr, sr * 4, 4, 32) + b'data'
                + struct.pack('<I', len(body)) + body)


def _signal(rng, n, sr, amp):
    t = np.arange(n) / sr
    return (amp * (0.6 * np.sin(2 * np.pi * 440.0 * t) + 0.4 * np.sin(2 * np.pi * 1900.0 * t + 1.0)) + 0.02 * rng.standard_normal(n)).astype(np.float32)


def test_command_line(tmp_path):
    from nele_gan_amd import dataio, resample
    rng = _rng('test_command_line')
    src, dst = tmp_path / 'in', tmp_path / 'out'
    (src / 'sub').mkdir(parents=True)
    made = {}
    for sr, n in ((8000, 400), (44100, 2205), (48000, 1931)):
        for kind, amp in (('f32', 1.7 if sr == 48000 else 0.5), ('pcm', 0.5)):         # the 48 kHz float file clips on purpose
            name = os.path.join('sub', 'a%d_%s.wav' % (sr, kind)) if kind == 'pcm' else 'a%d_%s.wav' % (sr, kind)
            (_write_float32 if kind == 'f32' else _write_pcm16)(str(src / name), _signal(rng, n, sr, amp), sr)
            made[name] = (sr, n)
    assert resample.main(['--in', str(src), '--out', str(dst), '--batch', '2']) == 0
    with open(dst / 'resample_manifest.csv', newline='') as fh:
        rows = list(csv.reader(fh))
    assert tuple(rows[0]) == resample.MANIFEST_COLUMNS == ('name', 'sr_in', 'samples_in', 'samples_out', 'peak', 'clipped_samples')
    assert [r[0] for r in rows[1:]] == sorted(made)
    any_clipped = 0
    for r in rows[1:]:
        sr, n = made[r[0]]
        x, file_sr = dataio.read_wav(str(src / r[0]))
        assert file_sr == sr and len(x) == n
        y, n_out = resample.resample(torch.from_numpy(x).cuda().unsqueeze(0), [n], sr)
        y = y[0].cpu().numpy()
        got, out_sr = dataio.read_wav(str(dst / r[0]))
        assert out_sr == 16000 and len(got) == int(n_out[0]) == R.out_len(n, *resample.ratio(sr, 16000))
        codes = np.rint(got * 32768.0).astype(np.int16)
        assert np.array_equal(codes, dataio.pcm16_quantise(y))
        up, down = resample.ratio(sr, 16000)
        want = R.scipy_resample(x, up, down, resample.taps(up, down, *R.PRESETS['high'])).astype(np.float32)
        assert np.abs(codes.astype(np.int32) - dataio.pcm16_quantise(want).astype(np.int32)).max() <= 1
        clipped = int((np.abs(y) * np.float32(32767.0) > 32767.5).sum())
        assert (int(r[1]), int(r[2]), int(r[3]), int(r[5])) == (sr, n, len(got), clipped)
        np.testing.assert_allclose(float(r[4]), np.abs(y).max(), rtol=1e-6)
        any_clipped += clipped
        assert (clipped > 0) == (r[0] == 'a48000_f32.wav')
    assert any_clipped > 0


def test_command_line_rewrites_files_already_at_the_rate(tmp_path):
    from nele_gan_amd import dataio, resample
    src, dst = tmp_path / 'in', tmp_path / 'out'
    src.mkdir()
    x = _signal(_rng('rewrite'), 500, 16000, 0.5)
    _write_float32(str(src / 'a.wav'), x, 16000)
    assert resample.main(['--in', str(src), '--out', str(dst)]) == 0
    got, sr = dataio.read_wav(str(dst / 'a.wav'))
    assert sr == 16000 and np.array_equal(np.rint(got * 32768.0).astype(np.int16), dataio.pcm16_quantise(x))       # not filtered


def test_opt_in_switches(tmp_path):
    from nele_gan_amd import dataio, mixing, resample, room
    rng = _rng('test_opt_in_switches')
    pool_dir, other_dir, rir_dir = tmp_path / 'pool', tmp_path / 'other', tmp_path / 'rir'
    for d in (pool_dir, other_dir, rir_dir):
        d.mkdir()
    lens = (4800, 3000)
    for k, n in enumerate(lens):
        _write_pcm16(str(pool_dir / ('n%d.wav' % k)), _signal(rng, n, 48000, 0.3), 48000)
        _write_pcm16(str(other_dir / ('n%d.wav' % k)), _signal(rng, n, 48000, 0.3), 48000)
    pool = sorted(dataio.get_filepaths(str(pool_dir)))
    m = mixing.NoiseMixer(pool, resample=True)
    assert m.pool_lengths_host.tolist() == [1600, 1000] and tuple(m.pool.shape) == (2, 1600)
    for k, p in enumerate(pool):
        x, sr = dataio.read_wav(p)
        y, n = resample.resample(torch.from_numpy(x).cuda().unsqueeze(0), [len(x)], 48000)
        assert np.array_equal(_bits(m.pool[k, :int(n[0])].cpu().numpy()), _bits(y[0].cpu().numpy()))
        got, got_sr = dataio.load(p, sr=16000, resample=True)
        assert got_sr == 16000 and np.array_equal(_bits(got), _bits(y[0].cpu().numpy()))
    assert mixing.NoiseMixer(pool, resample=True).tag() == m.tag()
    assert mixing.NoiseMixer(sorted(dataio.get_filepaths(str(other_dir))), resample=True).tag() != m.tag()
    # a room impulse response carries the sampling period: gain sr_in / sr_out = 3
    h48 = (np.exp(-np.arange(2400) / 300.0) * rng.standard_normal(2400) * 0.02).astype(np.float32)
    h48[40] = 0.9
    _write_pcm16(str(rir_dir / 'hall.wav'), h48, 48000)
    bank = room.RirBank(str(rir_dir), resample=True)
    x, _ = dataio.read_wav(str(rir_dir / 'hall.wav'))
    xd = torch.from_numpy(x).cuda().unsqueeze(0)
    y3, n3 = resample.resample(xd, [len(x)], 48000, gain=3.0)
    y1, _ = resample.resample(xd, [len(x)], 48000)
    assert bank.names == ['hall'] and len(bank.rirs[0]) == int(n3[0]) == 800
    assert np.array_equal(_bits(bank.rirs[0]), _bits(y3[0].cpu().numpy()))
    np.testing.assert_allclose(bank.rirs[0], 3.0 * y1[0].cpu().numpy(), rtol=2.0 ** -22, atol=1e-12)
    assert bank.b[0] == int(np.argmax(bank.rirs[0])) and abs(bank.b[0] - 40 / 3.0) <= 1
