"""A bulk-delay search that follows the delay when it moves after the lock.  On a real device the delay that ``BulkDelay`` finds is not
constant: every buffer under-run, route change or restarted audio stack moves it by whole buffers, and a canceller aligned to the old
delay cancels nothing.  ``TrackingBulkDelay`` is ``BulkDelay`` with its search started again from a cleared state behind every lock, over
and over: a background search that locks where the slot already is confirms the delay, one that locks elsewhere moves it, one that has
not locked after `patience` hops gives up; each is followed by `rest` hops without search work.  ``TrackedEchoCanceller`` puts it in
front of an ``EchoCanceller`` and restarts the canceller's weights in the slots whose delay moved, from a mask that never leaves the
device.  The kernels are in libnele_hip.so (csrc/bulktrack.hip, the ``nele_track_*`` entry points of include/nele_hip_track.h; the
arithmetic is DESIGN.md section 18, the search itself section 16's).  This module owns memory and bookkeeping only; there is no
arithmetic in torch.

    track = TrackingBulkDelay(streams=256, blocks=32)           # delays up to 32 * 256 - 1 samples (512 ms)
    aligned = track.process(mic_hops, played_hops)              # [256, nh * 256]: zeros before a slot's first lock, then `played` delayed
    track.delays(), track.moves()                               # int32 [256] on the device

    aec = TrackedEchoCanceller(track, EchoCanceller(256, partitions=4))
    loop = EchoCancellingEnhancer(RealtimeEnhancer(...), aec)   # as with a bare EchoCanceller
"""
import numpy as np
import torch

from . import _lib
from ._lib import c_longlong, call, ptr, stream
from ._slots import SlotState, to_dev

HOP = 256
MAX_BLOCKS = _lib.CONSTS['NELE_BULK_MAX_BLOCKS']
INFO = _lib.CONSTS['NELE_TRACK_INFO']
_FIELDS = (('delay', 'NELE_TRACK_I_DELAY'), ('hops', 'NELE_TRACK_I_HOPS'), ('age', 'NELE_TRACK_I_AGE'), ('sleep', 'NELE_TRACK_I_SLEEP'),
           ('moves', 'NELE_TRACK_I_MOVES'), ('confirms', 'NELE_TRACK_I_CONFIRMS'), ('gaveups', 'NELE_TRACK_I_GAVEUPS'),
           ('last_move', 'NELE_TRACK_I_LAST_MOVE'))


class TrackingBulkDelay(SlotState):
    """B independent delay searches that go on behind the lock.  blocks, lam, ratio, hold: ``BulkDelay``'s; patience (>= 1): the hops a
    background search of a locked slot is given to lock before it is dropped and begun again; rest (>= 0): hops without search work
    after every lock, confirmation, move and give-up."""

    def __init__(self, streams, blocks=32, lam=0.99, ratio=8.0, hold=16, patience=128, rest=0, device='cuda'):
        super().__init__(streams)
        self.Q = int(blocks)
        if not 2 <= self.Q <= MAX_BLOCKS:
            raise ValueError("TrackingBulkDelay: blocks must be in 2 .. %d (got %d)" % (MAX_BLOCKS, self.Q))
        self.lam, self.ratio, self.hold = float(lam), float(ratio), int(hold)
        if not (0.0 < self.lam < 1.0) or not (1.0 < self.ratio < float('inf')) or self.hold < 1:
            raise ValueError("TrackingBulkDelay: needs 0 < lam < 1, ratio > 1 and hold >= 1 (got %g, %g, %d)" % (self.lam, self.ratio, self.hold))
        self.patience, self.rest = int(patience), int(rest)
        if self.patience < 1 or self.rest < 0:
            raise ValueError("TrackingBulkDelay: needs patience >= 1 and rest >= 0 (got %d, %d)" % (self.patience, self.rest))
        self._alloc(device, _lib.lib.nele_track_state_bytes(self.S, self.Q))
        call('nele_track_init', ptr(self.state), c_longlong(self.nbytes), self.S, self.Q, stream())

    # ---- streaming
    def process(self, mic, played, active=None, out=None, want_moved=False):
        """mic, played [streams, nh * 256] float32 (host, pinned host or device) -> aligned [streams, nh * 256] on the device: exact zeros
        before a slot's first lock, then `played` of delays() hops ago, bit for bit.  active, out: as in ``BulkDelay.process``.
        want_moved: -> (aligned, moved), moved uint8 [streams] on the device: 1 for an active slot whose delay moved (a first lock is
        no move) during this call, 0 for every other slot.  Never blocks the host."""
        shape = tuple(np.shape(mic))
        if len(shape) != 2 or shape[0] != self.S or shape[1] % HOP or shape[1] == 0:
            raise ValueError("TrackingBulkDelay.process: mic must be [%d, nh * 256]" % self.S)
        nh = shape[1] // HOP
        d = self._dev_f32(mic, shape, 'mic')
        x = self._dev_f32(played, shape, 'played')
        act = None if active is None else self._flags(active, "TrackingBulkDelay: active must hold one flag per stream")
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float32:
            raise ValueError("TrackingBulkDelay.process: out must be float32 %s" % (shape,))
        moved = torch.empty((self.S,), dtype=torch.uint8, device=self.device) if want_moved else None
        call('nele_track_hop', ptr(self.state), c_longlong(self.nbytes), self.S, self.Q, ptr(d), ptr(x),
             ptr(None if act is None else self._dev_bytes(act)), nh, self.lam, self.ratio, self.hold, self.patience, self.rest, ptr(out), ptr(moved),
             stream())
        self.hops[slice(None) if act is None else act] += nh
        return (out, moved) if want_moved else out

    def status(self):
        """-> dict of device tensors: int32 [streams] each 'delay' (hops, -1 before the first lock), 'hops' (seen), 'age' (hops the
        current background search has seen), 'sleep' (hops left to rest), 'moves', 'confirms', 'gaveups', 'last_move' (the slot's hop
        index of the last move, -1 if none); 'energies' float64 [streams, blocks] and 'conf' float64 [streams] of the last hop a search
        of the slot evaluated (zeros before the first)."""
        info = torch.empty((self.S, INFO), dtype=torch.int32, device=self.device)
        st = {'energies': torch.empty((self.S, self.Q), dtype=torch.float64, device=self.device),
              'conf': torch.empty((self.S,), dtype=torch.float64, device=self.device)}
        call('nele_track_status', ptr(self.state), c_longlong(self.nbytes), self.S, self.Q, ptr(info), ptr(st['energies']), ptr(st['conf']), stream())
        for name, const in _FIELDS:
            st[name] = info[:, _lib.CONSTS[const]].contiguous()
        return st

    def _info(self, const):
        info = torch.empty((self.S, INFO), dtype=torch.int32, device=self.device)
        call('nele_track_status', ptr(self.state), c_longlong(self.nbytes), self.S, self.Q, ptr(info), None, None, stream())
        return info[:, _lib.CONSTS[const]].contiguous()

    def delays(self):
        """-> int32 [streams] on the device: each slot's delay in hops, -1 before its first lock"""
        return self._info('NELE_TRACK_I_DELAY')

    def moves(self):
        """-> int32 [streams] on the device: how often each slot's delay has moved since its reset"""
        return self._info('NELE_TRACK_I_MOVES')

    def set_delay(self, slots, hops):
        """Lock the given slots at delays the integrator knows: hops, one int in 0 .. blocks - 1 for all of them or one per slot.  Their
        background search starts from a cleared state; delay lines and counters are kept."""
        slots = np.asarray(slots, dtype=np.int64).reshape(-1)
        h = np.broadcast_to(np.asarray(hops, dtype=np.int64).reshape(-1), slots.shape) if np.size(hops) in (1, slots.size) else None
        if h is None or (h < 0).any() or (h >= self.Q).any():
            raise ValueError("TrackingBulkDelay.set_delay: hops must be one value, or one per slot, in 0 .. %d" % (self.Q - 1))
        m = self._slots_mask(slots)
        full = np.zeros(self.S, dtype=np.int32)
        full[slots] = h
        flags, delays = self._dev_bytes(m), to_dev(torch.from_numpy(full), self.device)     # both alive until the call has been enqueued
        call('nele_track_set_delay', ptr(self.state), c_longlong(self.nbytes), self.S, self.Q, ptr(flags), ptr(delays), stream())

    def reset(self, slots):
        """Restart the given slots (an empty delay line, no delay, zero counters); the other slots are not touched."""
        m = self._slots_mask(slots)
        call('nele_track_reset', ptr(self.state), c_longlong(self.nbytes), self.S, self.Q, ptr(self._dev_bytes(m)), stream())
        self.hops[m] = 0


class TrackedEchoCanceller:
    """``EchoCanceller`` behind a ``TrackingBulkDelay``: process() is aec.process(mic, track.process(mic, played, active), ...).  With
    reset_on_move the canceller is first restarted (``EchoCanceller.reset_flagged``) in the slots whose delay moved in this call, from
    the tracker's device mask and without a host read-back: weights fitted to the old alignment are worth nothing and would add a wrong
    echo estimate to the residual.  The canceller restarts at the first hop of the call in which the move fell, so with several hops per
    call the composite's bits depend on how the hops around a move are grouped into calls; the tracker's own bits do not.  (The
    canceller's host counter ``hops`` is not told of such a restart.)  A ``ResidualEchoSuppressor`` behind it is not reset: its smoothed
    spectra recover in a few hops.  Stands wherever an EchoCanceller does (``EchoCancellingEnhancer``, ``SuppressedEchoCanceller``,
    ``RateAdaptedEnhancer``)."""

    def __init__(self, track, aec, reset_on_move=True):
        if track.S != aec.S:
            raise ValueError("TrackedEchoCanceller: the delay tracker has %d streams, the canceller %d" % (track.S, aec.S))
        self.track, self.aec, self.S, self.device, self.P = track, aec, aec.S, aec.device, aec.P
        self.reset_on_move = bool(reset_on_move)

    def process(self, mic, played, active=None, adapt=None, want_echo=False, out=None):
        """EchoCanceller.process on `played` delayed by what the tracker holds (zeros before the first lock)"""
        if self.reset_on_move:
            aligned, moved = self.track.process(mic, played, active=active, want_moved=True)
            self.aec.reset_flagged(moved)
        else:
            aligned = self.track.process(mic, played, active=active)
        return self.aec.process(mic, aligned, active=active, adapt=adapt, want_echo=want_echo, out=out)

    def echo_path(self, slots=None):
        """EchoCanceller.echo_path: the path from the ALIGNED `played` to the microphone"""
        return self.aec.echo_path(slots)

    def reset(self, slots):
        """Restart the given slots in both objects: they search again."""
        self.track.reset(slots)
        self.aec.reset(slots)
