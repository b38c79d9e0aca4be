"""A bulk-delay search that follows the delay when it moves after the lock.  On a real device the delay that ``BulkDelay`` finds is not
constant: every buffer under-run, route change or restarted audio stack moves it by whole buffers, and a canceller aligned to the old
delay cancels nothing.  ``TrackingBulkDelay`` is ``BulkDelay`` with its search started again from a cleared state behind every lock, over
and over: a background search that locks where the slot already is confirms the delay, one that locks elsewhere moves it, one that has
not locked after `patience` hops gives up; each is followed by `rest` hops without search work.  ``TrackedEchoCanceller`` puts it in
front of an ``EchoCanceller`` and restarts the canceller's weights in the slots whose delay moved, from a mask that never leaves the
device.  The kernels are in libnele_hip.so (the tracking mode of csrc/bulkdelay.hip, the ``nele_track_*`` entry points of
include/nele_hip_ext.h; the arithmetic is DESIGN.md section 18, the search itself section 16's).  Both classes build on
nele_gan_amd/bulkdelay.py's: what is here is what differs.  This module owns memory and bookkeeping only; there is no arithmetic in
torch.

    track = TrackingBulkDelay(streams=256, blocks=32)           # delays up to 32 * 256 - 1 samples (512 ms)
    aligned = track.process(mic_hops, played_hops)              # [256, nh * 256]: zeros before a slot's first lock, then `played` delayed
    track.delays(), track.moves()                               # int32 [256] on the device

    aec = TrackedEchoCanceller(track, EchoCanceller(256, partitions=4))
    loop = EchoCancellingEnhancer(RealtimeEnhancer(...), aec)   # as with a bare EchoCanceller
"""
import torch

from . import _lib
from ._lib import ptr
from .bulkdelay import HOP, MAX_BLOCKS, AlignedEchoCanceller, BulkDelay

INFO = _lib.CONSTS['NELE_TRACK_INFO']
_FIELDS = (('delay', 'NELE_TRACK_I_DELAY'), ('hops', 'NELE_TRACK_I_HOPS'), ('age', 'NELE_TRACK_I_AGE'), ('sleep', 'NELE_TRACK_I_SLEEP'),
           ('moves', 'NELE_TRACK_I_MOVES'), ('confirms', 'NELE_TRACK_I_CONFIRMS'), ('gaveups', 'NELE_TRACK_I_GAVEUPS'),
           ('last_move', 'NELE_TRACK_I_LAST_MOVE'))


class TrackingBulkDelay(BulkDelay):
    """B independent delay searches that go on behind the lock.  blocks, lam, ratio, hold: ``BulkDelay``'s; patience (>= 1): the hops a
    background search of a locked slot is given to lock before it is dropped and begun again; rest (>= 0): hops without search work
    after every lock, confirmation, move and give-up.  set_delay() and reset() are ``BulkDelay``'s."""
    _ABI = 'nele_track'

    def __init__(self, streams, blocks=32, lam=0.99, ratio=8.0, hold=16, patience=128, rest=0, device='cuda'):
        self._settings(streams, blocks, lam, ratio, hold)
        self.patience, self.rest = int(patience), int(rest)
        if self.patience < 1 or self.rest < 0:
            raise ValueError("TrackingBulkDelay: needs patience >= 1 and rest >= 0 (got %d, %d)" % (self.patience, self.rest))
        self._lay_out(device)

    # ---- streaming
    def process(self, mic, played, active=None, out=None, want_moved=False):
        """mic, played [streams, nh * 256] float32 (host, pinned host or device) -> aligned [streams, nh * 256] on the device: exact zeros
        before a slot's first lock, then `played` of delays() hops ago, bit for bit.  active, out: as in ``BulkDelay.process``.
        want_moved: -> (aligned, moved), moved uint8 [streams] on the device: 1 for an active slot whose delay moved (a first lock is
        no move) during this call, 0 for every other slot.  Never blocks the host."""
        _, nh, d, x, act, flags, out = self._hop_args(mic, played, ('mic', 'played'), active, out)
        moved = torch.empty((self.S,), dtype=torch.uint8, device=self.device) if want_moved else None
        self._call('hop', ptr(d), ptr(x), ptr(flags), nh, self.lam, self.ratio, self.hold, self.patience, self.rest, ptr(out), ptr(moved))
        self._count(act, nh)
        return (out, moved) if want_moved else out

    def status(self):
        """-> dict of device tensors: int32 [streams] each 'delay' (hops, -1 before the first lock), 'hops' (seen), 'age' (hops the
        current background search has seen), 'sleep' (hops left to rest), 'moves', 'confirms', 'gaveups', 'last_move' (the slot's hop
        index of the last move, -1 if none); 'energies' float64 [streams, blocks] and 'conf' float64 [streams] of the last hop a search
        of the slot evaluated (zeros before the first)."""
        info = torch.empty((self.S, INFO), dtype=torch.int32, device=self.device)
        st = {'energies': torch.empty((self.S, self.Q), dtype=torch.float64, device=self.device),
              'conf': torch.empty((self.S,), dtype=torch.float64, device=self.device)}
        self._call('status', ptr(info), ptr(st['energies']), ptr(st['conf']))
        for name, const in _FIELDS:
            st[name] = info[:, _lib.CONSTS[const]].contiguous()
        return st

    def _info(self, const):
        info = torch.empty((self.S, INFO), dtype=torch.int32, device=self.device)
        self._call('status', ptr(info), None, None)
        return info[:, _lib.CONSTS[const]].contiguous()

    def delays(self):
        """-> int32 [streams] on the device: each slot's delay in hops, -1 before its first lock"""
        return self._info('NELE_TRACK_I_DELAY')

    def moves(self):
        """-> int32 [streams] on the device: how often each slot's delay has moved since its reset"""
        return self._info('NELE_TRACK_I_MOVES')


class TrackedEchoCanceller(AlignedEchoCanceller):
    """``EchoCanceller`` behind a ``TrackingBulkDelay``: process() is aec.process(mic, track.process(mic, played, active), ...).  With
    reset_on_move the canceller is first restarted (``EchoCanceller.reset_flagged``) in the slots whose delay moved in this call, from
    the tracker's device mask and without a host read-back: weights fitted to the old alignment are worth nothing and would add a wrong
    echo estimate to the residual.  The canceller restarts at the first hop of the call in which the move fell, so with several hops per
    call the composite's bits depend on how the hops around a move are grouped into calls; the tracker's own bits do not.  (The
    canceller's host counter ``hops`` is not told of such a restart.)  A ``ResidualEchoSuppressor`` behind it is not reset: its smoothed
    spectra recover in a few hops.  Stands wherever an EchoCanceller does (``EchoCancellingEnhancer``, ``SuppressedEchoCanceller``,
    ``RateAdaptedEnhancer``).  The tracker is ``.track`` (and ``AlignedEchoCanceller``'s ``.bulk``)."""
    _BULK = 'delay tracker'

    def __init__(self, track, aec, reset_on_move=True):
        super().__init__(track, aec)
        self.track = track
        self.reset_on_move = bool(reset_on_move)

    def _aligned(self, mic, played, active):
        """`played` delayed by what the tracker holds (zeros before the first lock)"""
        if not self.reset_on_move:
            return self.track.process(mic, played, active=active)
        aligned, moved = self.track.process(mic, played, active=active, want_moved=True)
        self.aec.reset_flagged(moved)
        return aligned
