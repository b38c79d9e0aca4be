"""The delay tracker of DESIGN.md section 18 restated in numpy, one stream at a time: the delay line of section 16, and behind it
section 16's search (tests/bulk_ref.py's BulkRef, used for its search state and step alone) started again from a cleared state after
every lock, confirmation, move and give-up.  Written from that section, not from csrc/bulkdelay.hip; tests/test_track_cpu.py checks it
on its own, tests/test_track_gpu.py holds the kernel to it."""
import numpy as np

from bulk_ref import HOP, BulkRef


class TrackRef:
    def __init__(self, blocks, lam=0.99, ratio=8.0, hold=16, patience=128, rest=0):
        self.Q, self.lam, self.ratio, self.hold = int(blocks), float(lam), float(ratio), int(hold)
        self.patience, self.rest = int(patience), int(rest)
        self.reset()

    def reset(self):
        self.line = np.zeros((self.Q, HOP), dtype=np.float32)          # line[k]: `played` of k hops ago
        self.delay, self.age, self.sleep, self.hops = -1, 0, 0, 0
        self.moves, self.confirms, self.gaveups, self.last_move = 0, 0, 0, -1
        self.e, self.conf = np.zeros(self.Q), 0.0                       # of the last evaluated hop: a clear leaves them
        self.events = []                                                # (hop, 'lock' | 'confirm' | 'move' | 'gaveup', q* or -1, delay after)
        self.log = []                                                   # BulkRef's log entries of every evaluated hop, with the slot's hop index in front
        self._clear()

    def _clear(self):
        self.bg = BulkRef(self.Q, self.lam, self.ratio, self.hold)      # its delay line and delay are not used

    def set_delay(self, h):
        if 0 <= h < self.Q:
            self.delay = int(h)
            self._clear()
            self.age, self.sleep = 0, 0

    def hop(self, d, x):
        """mic d [256], played x [256] float32 -> (aligned [256] float32, moved: did a move fall on this hop)"""
        x32 = np.asarray(x, dtype=np.float32)
        self.line = np.roll(self.line, 1, axis=0)
        self.line[0] = x32
        moved = False
        if self.sleep > 0:
            self.sleep -= 1
        else:
            bg = self.bg
            seen = len(bg.log)
            bg._search(np.asarray(d, dtype=np.float64), x32.astype(np.float64))
            self.age += 1
            hit = False
            if len(bg.log) > seen:                                      # the hop was evaluated
                self.e, self.conf = bg.e.copy(), bg.conf
                self.log.append((self.hops,) + bg.log[-1])
                hit = bg.run_len >= self.hold
            done = None
            if hit:
                qs = bg.log[-1][1]
                if self.delay < 0:
                    self.delay, done = max(qs - 1, 0), 'lock'
                elif 0 <= qs - self.delay <= 2:
                    self.confirms, done = self.confirms + 1, 'confirm'
                else:
                    self.delay, done = max(qs - 1, 0), 'move'
                    self.moves, self.last_move, moved = self.moves + 1, self.hops, True
                self.events.append((self.hops, done, qs, self.delay))
            elif self.delay >= 0 and self.age >= self.patience:
                self.gaveups, done = self.gaveups + 1, 'gaveup'
                self.events.append((self.hops, done, -1, self.delay))
            if done is not None:
                self._clear()
                self.age, self.sleep = 0, self.rest
        self.hops += 1
        y = np.zeros(HOP, np.float32) if self.delay < 0 else self.line[self.delay].copy()
        return y, moved

    def run(self, mic, played):
        """whole hops of mic / played [nh * 256] -> aligned [nh * 256] float32"""
        return np.concatenate([self.hop(mic[i:i + HOP], played[i:i + HOP])[0] for i in range(0, len(mic) // HOP * HOP, HOP)])

    def of(self, kind):
        return [ev for ev in self.events if ev[1] == kind]
