"""What a move of the delay tracker costs the drift-compensated echo path, on the CPU references (minutes; DESIGN.md section 19 quotes
it): python tools/drift_move.py [--ppm 500] [--hops 3300] [--bulk 1500] [--blocks 8] [--ratio 3.0] [--start-ppm 0]

tests/track_ref.py (locked by set_delay at the known base), tests/drift_ref.py and tests/aec_ref.py (P = 4) chained one hop per call
on tests/drift_cases.py's scenario (ENR 10 dB, path 700 taps / 0.08 s): the capture clock runs fast, the echo's delay shrinks by ppm
256e-6 samples per hop, tau follows it until the main tap has left the 768 samples the tracker promises; the tracker then moves by
whole hops, the compensator snaps (rate kept) and the canceller restarts.  Printed: the tracker's events, tau, the estimate and the echo
reduction per 300-hop window - beside the same chain without the compensator."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np  # noqa: E402

import drift_cases as DC  # noqa: E402
from aec_ref import AecRef  # noqa: E402
from drift_ref import HOP, DriftRef  # noqa: E402
from track_ref import TrackRef  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ppm', type=float, default=500.0)
    ap.add_argument('--hops', type=int, default=3300)
    ap.add_argument('--bulk', type=int, default=1500)
    ap.add_argument('--blocks', type=int, default=8)
    ap.add_argument('--ratio', type=float, default=3.0, help="the tracker's ratio (at 500 ppm its confidence stays below the default 8)")
    ap.add_argument('--start-ppm', type=float, default=0.0, help='the estimate the compensator starts from (set_rate)')
    a = ap.parse_args()
    s = DC.scenario(a.ppm, 10.0, 1, a.hops, bulk=a.bulk)
    base = max((a.bulk + 40) // HOP - 1, 0)
    chains = {}
    for name in ('compensated', 'whole hops only'):
        tr = TrackRef(a.blocks, ratio=a.ratio)
        tr.set_delay(base)
        chains[name] = {'track': tr, 'drift': DriftRef(a.blocks), 'aec': AecRef(4), 'y': [], 'log': []}
        chains[name]['drift'].set_rate(-1e-6 * a.start_ppm)
    for k in range(a.hops):
        d, x = s['mic'][k * HOP:(k + 1) * HOP], s['played'][k * HOP:(k + 1) * HOP]
        for name, c in chains.items():
            whole, moved = c['track'].hop(d, x)
            snapped = c['drift'].begin_call(c['track'].delay)
            al = c['drift'].hop(d, x)
            if name != 'compensated':
                al = whole
            if (snapped if name == 'compensated' else moved) and k:
                c['aec'] = AecRef(4)
                c['log'].append((k, c['track'].delay))
            c['y'].append(c['aec'].hop(d, al)[1])
            if name == 'compensated' and (k % 300 == 299 or snapped):
                print('hop %5d: delay %d hops, tau %8.2f (the echo is %8.2f samples late), estimate %7.2f ppm%s'
                      % (k, c['track'].delay, c['drift'].tau, a.bulk + 40 - (k + 1) * HOP * a.ppm * 1e-6, c['drift'].drift_ppm, ', SNAP' if snapped else ''),
                      flush=True)
    for name, c in chains.items():
        y = np.concatenate(c['y'])
        ev = c['track'].events
        print('%s: restarts of the canceller at (hop, new delay) %s; the tracker confirmed %d times; its other events %s'
              % (name, c['log'], len([e for e in ev if e[1] == 'confirm']), [(e[0], e[1], e[3]) for e in ev if e[1] != 'confirm']))
        print('  echo reduction per 300 hops: ' + ' '.join('%.1f' % DC.window_db(s['echo'], y, w, w + 300) for w in range(0, a.hops - 299, 300)))


if __name__ == '__main__':
    main()
