"""Room impulse responses without a measured database: shoebox rooms by the image-source method, synthesised on the GPU
(csrc/roomsynth.hip; the definition is DESIGN.md section 13).  Neither the reference nor its corpus ships a room: an addition.

    synth_rirs(rooms, taps)                   -> (h float64 [R, N], status int32 [R]) on the device        nele_rir_synth
    t60_of(h, fs)                             -> decay time from the Schroeder energy decay curve (-5 .. -25 dB, times 3)
    draw_rooms(n, seed, ...)                  -> n rooms, room i a function of (seed, i) alone
    synth_bank(n, seed, ...)                  -> room.RirBank 'synth0000' ..., each room calibrated to its target T60, and a resolver
                                                 that gives every file its room
    python -m nele_gan_amd.roomsynth --rooms N --seed S --out DIR [--t60 lo hi]
                                              DIR/rooms.json and one 16 kHz PCM_16 wav per room (peak 0.9): a folder for --rir
"""
import collections
import json
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream
from .mixing import draw_words

BAD_SIZE, BAD_POSITION, BAD_BETA = (_lib.CONSTS['NELE_RIR_BAD_' + _n] for _n in ('SIZE', 'POSITION', 'BETA'))
FS, C, HALF_WIDTH = 16000, 343.0, 40


def library():
    """-> the loaded libnele_hip.so (ctypes), every entry point bound"""
    return _lib.lib


def __getattr__(name):
    if name == 'TILE':                                     # taps per workgroup of the kernel (tests put lengths around it)
        return int(_lib.lib.nele_rir_synth_tile())
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


Shoebox = collections.namedtuple('Shoebox', 'L s m beta')   # sizes [3], source [3], receiver [3] (m), beta [3][2] (wall at 0, wall at L)


def room_row(room):
    """Shoebox (or 15 numbers) -> the 15 numbers of the C ABI's room record: L, s, m, beta[x][0], beta[x][1], beta[y][0], ..."""
    if isinstance(room, Shoebox):
        room = list(room.L) + list(room.s) + list(room.m) + [b for pair in room.beta for b in pair]
    row = np.asarray(room, dtype=np.float64).reshape(-1)
    if row.shape != (15,):
        raise ValueError("roomsynth: a room is 15 numbers (3 sizes, source, receiver, 6 reflection factors), got %d" % row.size)
    return row


def shoebox_of(row):
    row = room_row(row)
    return Shoebox(tuple(row[0:3]), tuple(row[3:6]), tuple(row[6:9]), tuple((row[9 + 2 * a], row[10 + 2 * a]) for a in range(3)))


def synth_rirs(rooms, taps, fs=FS, c=C, half_width=HALF_WIDTH, device='cuda', N=None):
    """rooms: array [R, 15] or a list of Shoebox; taps: an int or one per room -> (h float64 [R, N] with exact zeros behind taps[r],
    status int32 [R]: 0 or BAD_* bits, and then a zero row), both on the device.  N: the row length (default: the largest taps)."""
    rows = np.stack([room_row(r) for r in rooms]) if not isinstance(rooms, np.ndarray) else np.asarray(rooms, dtype=np.float64)
    if rows.ndim != 2 or rows.shape[1] != 15 or rows.shape[0] == 0:
        raise ValueError("roomsynth: rooms must be [R, 15]")
    R = rows.shape[0]
    t = np.full(R, int(taps), dtype=np.int32) if np.ndim(taps) == 0 else np.asarray(taps, dtype=np.int32).reshape(-1)
    if t.shape != (R,) or (t < 1).any():
        raise ValueError("roomsynth: taps must be positive, one per room")
    N = int(t.max()) if N is None else int(N)
    if (t > N).any():
        raise ValueError("roomsynth: taps above N=%d" % N)
    packed = np.zeros((R, 16), dtype=np.float64)
    packed[:, :15] = rows
    dev = torch.device(device)
    d_rooms, d_taps = torch.from_numpy(packed).to(dev), torch.from_numpy(t).to(dev)
    h = torch.empty((R, N), dtype=torch.float64, device=dev)
    status = torch.empty((R,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        call('nele_rir_synth', ptr(d_rooms), ptr(d_taps), R, N, float(fs), float(c), int(half_width), ptr(h), ptr(status), None, stream())
        torch.cuda.current_stream().synchronize()            # d_rooms / d_taps die here
    return h, status


def t60_of(h, fs=FS):
    """Decay time of h [N] or [R, N] (torch tensor, any device) from the Schroeder energy decay curve E[n] = sum_{k >= n} h[k]^2 in dB
    relative to E[0]: three times the span between its -5 dB and -25 dB crossings (each linearly interpolated between the last sample
    above the level and the first at or below it).  -> float64 tensor [R] (or a 0-d tensor) of seconds; NaN for an all-zero row."""
    x = h.double()
    one = x.dim() == 1
    if one:
        x = x[None, :]
    e = torch.flip(torch.cumsum(torch.flip(x * x, dims=[1]), dim=1), dims=[1])
    db = 10.0 * torch.log10(e / e[:, :1])
    n = x.shape[1]

    def crossing(level):
        below = db <= level
        i = torch.where(below.any(dim=1), below.int().argmax(dim=1), torch.full((x.shape[0],), n, device=x.device))     # first at or below
        hi = torch.gather(db, 1, torch.clamp(i - 1, 0, n - 1)[:, None])[:, 0]
        lo = torch.where(i < n, torch.gather(db, 1, torch.clamp(i, max=n - 1)[:, None])[:, 0], torch.full_like(hi, -math.inf))
        frac = torch.where(torch.isinf(lo), torch.zeros_like(hi), (hi - level) / (hi - lo))
        return (i - 1).double() + frac
    t = 3.0 * (crossing(-25.0) - crossing(-5.0)) / float(fs)
    return t[0] if one else t


def _unit(word):
    return word / 18446744073709551616.0                    # [0, 1)


def draw_rooms(n, seed, size_m=((3, 10), (3, 8), (2.4, 4)), t60_s=(0.2, 0.8), min_dist_m=0.5, margin_m=0.3):
    """-> n dicts {'room': Shoebox, 't60_target': seconds}.  Room i is a function of (seed, i) alone (mixing.draw_words: counter-based,
    like the noise draws).  Sizes, source, receiver and the target T60 are uniform in their ranges; source and receiver keep margin_m
    from every wall and min_dist_m from each other (positions are drawn again, under the next counter, until they do); every wall gets
    the reflection factor Eyring's formula gives for the target: ln beta = -0.5 * 0.161 V / (S T60)."""
    out = []
    for i in range(int(n)):
        key = 'room:%d' % i
        w = draw_words(seed, key, 0, n=4)
        L = tuple(lo + (hi - lo) * _unit(w[a]) for a, (lo, hi) in enumerate(size_m))
        t60 = t60_s[0] + (t60_s[1] - t60_s[0]) * _unit(w[3])
        if min(L) <= 2 * margin_m:
            raise ValueError("draw_rooms: margin_m=%g leaves no space in a room of %s m" % (margin_m, L))
        for attempt in range(1, 1001):
            p = [_unit(v) for v in draw_words(seed, key, attempt, n=6)]
            s = tuple(margin_m + (L[a] - 2 * margin_m) * p[a] for a in range(3))
            m = tuple(margin_m + (L[a] - 2 * margin_m) * p[3 + a] for a in range(3))
            if math.dist(s, m) >= min_dist_m:
                break
        else:
            raise ValueError("draw_rooms: no source / receiver %g m apart in a room of %s m" % (min_dist_m, L))
        V, S = L[0] * L[1] * L[2], 2.0 * (L[0] * L[1] + L[1] * L[2] + L[0] * L[2])
        beta = math.exp(-0.5 * 0.161 * V / (S * t60))
        out.append({'room': Shoebox(L, s, m, ((beta, beta),) * 3), 't60_target': t60})
    return out


def room_resolver(n, seed, p_dry=0.0):
    """file name -> 'synthNNNN', the room w[0] mod n of w = mixing.draw_words(seed, base name, 0) (its default three words), or None - an
    anechoic row - where w[1] / 2^64 < p_dry: a function of (seed, base name) alone - the same on every rank, in every batch and on every
    run."""
    def resolve(file_name):
        w = draw_words(seed, os.path.basename(str(file_name)), 0)
        if _unit(w[1]) < p_dry:
            return None
        return 'synth%04d' % (w[0] % n)
    return resolve


def _measure(hs, fs):
    if torch.is_tensor(hs):
        return t60_of(hs, fs).cpu().numpy()
    return np.asarray([float(t60_of(torch.from_numpy(np.asarray(h, dtype=np.float64)), fs)) for h in hs])


def calibrate_rooms(drawn, synth, calibrate=2, fs=FS, max_taps=16000):
    """The calibration loop on any synthesiser: synth(list of Shoebox, taps [R]) -> list of R responses (arrays or tensor rows).  A
    shoebox's image-source response decays more slowly than Eyring's formula predicts, so after each synthesis ln beta of every wall is
    scaled by measured T60 / target T60; ``calibrate`` rescales = calibrate + 1 synth calls.  -> (responses, rooms, measured T60 [R], taps [R])."""
    rooms = [d['room'] for d in drawn]
    target = np.asarray([d['t60_target'] for d in drawn], dtype=np.float64)
    taps = np.minimum(np.ceil(target * fs).astype(np.int64), int(max_taps)).astype(np.int32)
    for it in range(int(calibrate) + 1):
        hs = synth(rooms, taps)
        measured = _measure(hs, fs)
        if not np.isfinite(measured).all() or (measured <= 0).any():
            raise ValueError("synth_bank: a room's decay time cannot be measured (T60 %s)" % measured.tolist())
        if it < calibrate:
            rooms = [r._replace(beta=tuple(tuple(b ** (mt / tt) if b > 0 else 0.0 for b in pair) for pair in r.beta))
                     for r, mt, tt in zip(rooms, measured, target)]
    return hs, rooms, measured, taps


def synth_bank(n, seed, size_m=((3, 10), (3, 8), (2.4, 4)), t60_s=(0.2, 0.8), min_dist_m=0.5, margin_m=0.3, calibrate=2, p_dry=0.0, tau=32,
               max_taps=16000, fs=FS, device='cuda'):
    """-> room.RirBank of n synthesised rooms 'synth0000' ... (taps = min(ceil(T60 fs), max_taps)), each moved towards its drawn T60 by
    ``calibrate`` rescales of ln beta (calibrate + 1 kernel calls for the whole bank).  bank.rooms: per room its sizes, positions, final
    beta, target and measured T60; bank.resolver: room_resolver(n, seed, p_dry).
    How close: over 64 rooms at the default ranges two rescales end at a median of 1 % from the target, five rooms beyond 5 %, the
    worst 14.6 % - large rooms with a short T60 (0.24 .. 0.36 s in 9 x 5 x 3 m), where the direct sound and the first reflections carry
    most of the energy and the decay curve between -5 and -25 dB is a few steps, not a slope; more rescales bring the median to 0.15 %
    and leave such a room at 12 to 13 %.  The measured value is recorded per room: filter bank.rooms on it where that matters."""
    from . import room as _room
    drawn = draw_rooms(n, seed, size_m=size_m, t60_s=t60_s, min_dist_m=min_dist_m, margin_m=margin_m)

    def synth(rooms, taps):
        h, status = synth_rirs(rooms, taps, fs=fs, device=device)
        if int(status.abs().max()) != 0:
            raise ValueError("synth_bank: nele_rir_synth status %s" % status.cpu().tolist())
        return h
    h, rooms, measured, taps = calibrate_rooms(drawn, synth, calibrate=calibrate, fs=fs, max_taps=max_taps)
    host = h.cpu().numpy()
    names = ['synth%04d' % i for i in range(len(rooms))]
    bank = _room.RirBank({nm: host[i, :taps[i]] for i, nm in enumerate(names)}, tau=tau, resolver=room_resolver(len(rooms), seed, p_dry), device=device)
    bank.rooms = [{'name': nm, 'L': list(r.L), 's': list(r.s), 'm': list(r.m), 'beta': [list(p) for p in r.beta], 't60_target': float(d['t60_target']),
                   't60_measured': float(mt), 'taps': int(t)} for nm, r, d, mt, t in zip(names, rooms, drawn, measured, taps)]
    bank.seed, bank.p_dry = int(seed), float(p_dry)
    return bank


def export_bank(bank, out_dir, fs=FS):
    """bank.rooms and the responses -> out_dir/rooms.json and one PCM_16 wav per room, scaled to peak 0.9 (Room.apply renormalises after
    filtering, so the scale does not reach a score; rooms.json records it).  -> the list written to rooms.json."""
    from . import dataio
    dataio.creatdir(out_dir)
    listed = []
    for rec, h in zip(bank.rooms, bank.rirs):
        scale = 0.9 / float(np.max(np.abs(h)))
        dataio.write_wav_pcm16(os.path.join(out_dir, rec['name'] + '.wav'), (h.astype(np.float64) * scale).astype(np.float32), sr=fs)
        listed.append(dict(rec, scale=scale))
    with open(os.path.join(out_dir, 'rooms.json'), 'w') as fh:
        json.dump({'fs': fs, 'seed': getattr(bank, 'seed', None), 'tau': bank.tau, 'rooms': listed}, fh, indent=1)
    return listed


def add_cli_arguments(ap):
    """--rooms-synth N --rooms-seed S --rooms-t60 lo hi --rooms-dry p of the training and scoring entry points"""
    ap.add_argument('--rooms-synth', type=int, default=0, metavar='N', help='synthesise N shoebox rooms on the GPU and take the targets in the room each file '
                                                                           'name draws (instead of --rir: needs no database; excludes --rir).  A room\'s decay '
                                                                           'time ends within a few per cent of the one drawn for it, large rooms with a short one '
                                                                           'up to 15 %% off')
    ap.add_argument('--rooms-seed', type=int, default=0)
    ap.add_argument('--rooms-t60', type=float, nargs=2, default=(0.2, 0.8), metavar=('LO', 'HI'), help='range of the decay times drawn, seconds')
    ap.add_argument('--rooms-dry', type=float, default=0.0, metavar='P', help='share of the files that stay anechoic')


def bank_from_cli(ap, a, device='cuda'):
    """-> the RirBank of --rooms-synth ... or None; --rooms-synth and --rir exclude each other"""
    if not a.rooms_synth:
        return None
    if a.rir:
        ap.error('--rooms-synth and --rir exclude each other')
    if a.rooms_synth < 1 or not (0.0 < a.rooms_t60[0] <= a.rooms_t60[1]) or not (0.0 <= a.rooms_dry <= 1.0):
        ap.error('--rooms-synth needs N >= 1, 0 < lo <= hi for --rooms-t60 and --rooms-dry in 0 .. 1')
    return synth_bank(a.rooms_synth, a.rooms_seed, t60_s=tuple(a.rooms_t60), p_dry=a.rooms_dry, device=device)


def build_parser():
    import argparse
    ap = argparse.ArgumentParser(prog='python -m nele_gan_amd.roomsynth', description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--rooms', type=int, required=True, help='number of rooms')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', required=True, help='folder rooms.json and the wav files are written under')
    ap.add_argument('--t60', type=float, nargs=2, default=(0.2, 0.8), metavar=('LO', 'HI'), help='range of the decay times drawn, seconds')
    return ap


def parse_args(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.rooms < 1:
        ap.error('--rooms must be positive')
    if not (0.0 < a.t60[0] <= a.t60[1]):
        ap.error('--t60 needs 0 < lo <= hi')
    return a


def main(argv=None):
    a = parse_args(argv)
    bank = synth_bank(a.rooms, a.seed, t60_s=tuple(a.t60))
    listed = export_bank(bank, a.out)
    worst = max(abs(r['t60_measured'] / r['t60_target'] - 1.0) for r in listed)
    print('%d rooms under %s (T60 %.2f .. %.2f s, at most %.1f %% from the target)' % (len(listed), a.out.rstrip('/'), min(r['t60_measured'] for r in listed),
                                                                                    max(r['t60_measured'] for r in listed), 100.0 * worst))
    return 0


if __name__ == '__main__':
    import sys
    sys.exit(main())
