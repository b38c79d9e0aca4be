#!/usr/bin/env python
"""Device time of the image-source room synthesiser (csrc/roomsynth.hip) beside the numpy reference on one host core.

    python tools/roomsynth_time.py [--out profiles/roomsynth/roomsynth_time.json] [--reps 5] [--no-numpy]

Cases, each in a child process of its own under its own time limit (the parent opens no GPU; after a child that fails or runs out of
time nothing further is started):
    kernel_64     nele_rir_synth, 64 rooms drawn by draw_rooms(seed 1) with T60 in 0.2 .. 0.8 s, taps = ceil(T60 fs), Eyring's beta
    kernel_256    the same, 256 rooms
    one_room      one (5, 4, 3) m room, 0.3 s: the case the numpy reference is timed on
    bank_64       synth_bank(64, seed 1) with its two calibration rescales: three kernel calls, three t60_of, the host loop between them
Device times: HIP events around the call, median of --reps after one warm-up call.  images = the number of (image, tap) products / 81,
counted by the reference's enumeration for one_room only.  Host: tests/roomsynth_ref.py rir() of one_room, one pass, wall clock, one
thread."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = {'kernel_64': 120, 'kernel_256': 240, 'one_room': 60, 'bank_64': 240}      # name -> time limit of its child, seconds
ONE_ROOM = [5.0, 4.0, 3.0, 1.55, 1.68, 1.41, 3.1, 2.2, 1.5] + [0.85] * 6
ONE_ROOM_TAPS = 4800


def _events(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms)}


def run_case(name, reps):
    import numpy as np
    import torch
    from nele_gan_amd import _lib, roomsynth
    roomsynth.library()
    if name == 'bank_64':
        r = _events(lambda: roomsynth.synth_bank(64, seed=1), max(1, reps // 2))
        bank = roomsynth.synth_bank(64, seed=1)
        r['worst_t60_error'] = max(abs(x['t60_measured'] / x['t60_target'] - 1.0) for x in bank.rooms)
        r['taps_total'] = int(sum(x['taps'] for x in bank.rooms))
        return r
    if name == 'one_room':
        rows, taps = np.asarray([ONE_ROOM]), np.asarray([ONE_ROOM_TAPS], dtype=np.int32)
    else:
        drawn = roomsynth.draw_rooms(int(name.split('_')[1]), seed=1)
        rows = np.stack([roomsynth.room_row(d['room']) for d in drawn])
        taps = np.asarray([int(np.ceil(d['t60_target'] * 16000)) for d in drawn], dtype=np.int32)
    R, N = rows.shape[0], int(taps.max())
    packed = np.zeros((R, 16))
    packed[:, :15] = rows
    d_rooms, d_taps = torch.from_numpy(packed).cuda(), torch.from_numpy(taps).cuda()
    out = torch.empty((R, N), dtype=torch.float64, device='cuda')
    status = torch.empty((R,), dtype=torch.int32, device='cuda')
    r = _events(lambda: _lib.call('nele_rir_synth', _lib.ptr(d_rooms), _lib.ptr(d_taps), R, N, 16000.0, 343.0, 40, _lib.ptr(out), _lib.ptr(status), None,
                                  _lib.stream()), reps)
    assert int(status.abs().max()) == 0
    # images per room ~ (4 pi / 3) d^3 / V, d = (taps + 40) c / fs
    vol = rows[:, 0] * rows[:, 1] * rows[:, 2]
    images = float(((4.0 * np.pi / 3.0) * ((taps + 40) * 343.0 / 16000.0) ** 3 / vol).sum())
    r.update({'rooms': R, 'N': N, 'taps_total': int(taps.sum()), 'images_estimate': images, 'image_taps_per_s': images * 81 / (r['median_ms'] * 1e-3),
              'device': _lib.device_info()})
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'roomsynth', 'roomsynth_time.json'))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-numpy', action='store_true')
    ap.add_argument('--case', choices=sorted(CASES), default=None, help='(internal) run one case in this process and print its JSON line')
    a = ap.parse_args()
    if a.case:
        print('RESULT ' + json.dumps(run_case(a.case, a.reps)), flush=True)
        return 0
    res = {'reps': a.reps, 'cases': {}}
    for name, limit in CASES.items():
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--case', name, '--reps', str(a.reps)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                               text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print('%s: no result within %d s - stopping' % (name, limit), flush=True)
            return 1
        line = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')]
        if p.returncode != 0 or not line:
            print(p.stdout)
            print('%s: exit status %d - stopping' % (name, p.returncode), flush=True)
            return 1
        res['cases'][name] = json.loads(line[-1][7:])
        print(name, json.dumps(res['cases'][name]), flush=True)
    if not a.no_numpy:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import roomsynth_ref
        t0 = time.perf_counter()
        tau, _ = roomsynth_ref.images(ONE_ROOM, ONE_ROOM_TAPS)
        t1 = time.perf_counter()
        roomsynth_ref.rir(ONE_ROOM, ONE_ROOM_TAPS)
        res['numpy_one_room'] = {'seconds': time.perf_counter() - t1, 'enumeration_seconds': t1 - t0, 'images': int(len(tau)), 'taps': ONE_ROOM_TAPS}
        print('numpy_one_room', json.dumps(res['numpy_one_room']), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
    print('wrote', a.out)
    return 0


if __name__ == '__main__':
    sys.exit(main())
