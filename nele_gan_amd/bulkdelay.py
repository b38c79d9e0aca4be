"""Bulk-delay search and alignment ahead of the echo canceller: playback and capture buffers put 50 to 500 ms between what the loudspeaker
is handed and when the microphone hears it, far more than ``EchoCanceller``'s partitions should be spent on.  ``BulkDelay`` finds that
delay per stream slot in whole 256-sample hops - SCOT-weighted cross-spectra of the microphone against the last Q far-end blocks, on
the GPU, without a host read-back - and hands `played` on late by it; ``AlignedEchoCanceller`` puts it in front of an
``EchoCanceller``, which then needs partitions for the room's tail plus two blocks only.  The kernels are in libnele_hip.so
(csrc/bulkdelay.hip, the ``nele_bulk_*`` entry points of include/nele_hip_ext.h; the arithmetic is DESIGN.md section 16).  This module
owns memory and bookkeeping only; there is no arithmetic in torch.  nele_gan_amd/bulktrack.py builds the pair that follows a delay which
moves after the lock on these two classes.

    bulk = BulkDelay(streams=256, blocks=32)                    # delays up to 32 * 256 - 1 samples (512 ms)
    aligned = bulk.process(mic_hops, played_hops)               # [256, nh * 256]: zeros while a slot searches, then `played` delayed
    bulk.delays()                                               # int32 [256] on the device: hops, -1 = still searching

    aec = AlignedEchoCanceller(bulk, EchoCanceller(256, partitions=4))
    loop = EchoCancellingEnhancer(RealtimeEnhancer(...), aec)   # as with a bare EchoCanceller
"""
import numpy as np
import torch

from . import _lib
from ._lib import c_longlong, call, ptr, stream
from ._slots import HOP, SlotState, to_dev

MAX_BLOCKS = _lib.CONSTS['NELE_BULK_MAX_BLOCKS']


class BulkDelay(SlotState):
    """B independent delay searches.  blocks: Q in 2 .. 64, the search covers main-tap delays up to 256 Q - 1 samples; lam (0 < lam < 1):
    the decay per hop of the cross-spectrum sums; a slot locks once one block has held (Q - 1) times its energy >= ratio (> 1) times the
    sum of the others' for hold (>= 1) hops in a row, at that block less one."""
    _ABI = 'nele_bulk'                                     # the entry points are _ABI + '_init', '_hop', ...

    def __init__(self, streams, blocks=32, lam=0.99, ratio=8.0, hold=16, device='cuda'):
        self._settings(streams, blocks, lam, ratio, hold)
        self._lay_out(device)

    def _settings(self, streams, blocks, lam, ratio, hold):
        SlotState.__init__(self, streams)
        who = type(self).__name__
        self.Q = int(blocks)
        if not 2 <= self.Q <= MAX_BLOCKS:
            raise ValueError("%s: blocks must be in 2 .. %d (got %d)" % (who, MAX_BLOCKS, self.Q))
        self.lam, self.ratio, self.hold = float(lam), float(ratio), int(hold)
        if not (0.0 < self.lam < 1.0) or not (1.0 < self.ratio < float('inf')) or self.hold < 1:
            raise ValueError("%s: needs 0 < lam < 1, ratio > 1 and hold >= 1 (got %g, %g, %d)" % (who, self.lam, self.ratio, self.hold))

    def _lay_out(self, device):
        self._alloc(device, getattr(_lib.lib, self._ABI + '_state_bytes')(self.S, self.Q))
        self._call('init')

    def _call(self, what, *args):
        call('%s_%s' % (self._ABI, what), ptr(self.state), c_longlong(self.nbytes), self.S, self.Q, *args, stream())

    # ---- streaming
    def process(self, mic, played, active=None, out=None):
        """mic, played [streams, nh * 256] float32 (host, pinned host or device) -> aligned [streams, nh * 256] on the device: exact zeros
        while a slot searches, then `played` of delays() hops ago, bit for bit.  active: host bool sequence [streams] or None (all):
        inactive slots are neither read nor changed and their output columns are left as they were.  out: a buffer on the device to
        write into - the way to keep an inactive slot's columns; without it the output is a fresh tensor and an inactive slot's columns
        undefined.  Never blocks the host."""
        _, nh, d, x, act, flags, out = self._hop_args(mic, played, ('mic', 'played'), active, out)
        self._call('hop', ptr(d), ptr(x), ptr(flags), nh, self.lam, self.ratio, self.hold, ptr(out), None)
        self._count(act, nh)
        return out

    def status(self):
        """-> dict of device tensors: 'delay' int32 [streams] (hops, -1 = searching), 'hops_searched' int32 [streams], 'energies'
        float64 [streams, blocks] and 'conf' float64 [streams] of the last hop the search evaluated (zeros before the first)."""
        st = {'delay': torch.empty((self.S,), dtype=torch.int32, device=self.device),
              'hops_searched': torch.empty((self.S,), dtype=torch.int32, device=self.device),
              'energies': torch.empty((self.S, self.Q), dtype=torch.float64, device=self.device),
              'conf': torch.empty((self.S,), dtype=torch.float64, device=self.device)}
        self._call('status', ptr(st['delay']), ptr(st['hops_searched']), ptr(st['energies']), ptr(st['conf']))
        return st

    def delays(self):
        """-> int32 [streams] on the device: each slot's delay in hops, -1 while it searches"""
        d = torch.empty((self.S,), dtype=torch.int32, device=self.device)
        self._call('status', ptr(d), None, None, None)
        return d

    def set_delay(self, slots, hops):
        """Lock the given slots at delays the integrator knows: hops, one int in 0 .. blocks - 1 for all of them or one per slot.  Their
        delay lines are kept.  ``BulkDelay``: no search runs in them afterwards.  ``TrackingBulkDelay``: their background search starts
        from a cleared state; the counters are kept."""
        slots = np.asarray(slots, dtype=np.int64).reshape(-1)
        h = np.broadcast_to(np.asarray(hops, dtype=np.int64).reshape(-1), slots.shape) if np.size(hops) in (1, slots.size) else None
        if h is None or (h < 0).any() or (h >= self.Q).any():
            raise ValueError("%s.set_delay: hops must be one value, or one per slot, in 0 .. %d" % (type(self).__name__, self.Q - 1))
        m = self._slots_mask(slots)
        full = np.zeros(self.S, dtype=np.int32)
        full[slots] = h
        flags, delays = self._dev_bytes(m), to_dev(torch.from_numpy(full), self.device)     # both alive until the call has been enqueued
        self._call('set_delay', ptr(flags), ptr(delays))

    def reset(self, slots):
        """Restart the given slots (an empty delay line, the search from its beginning, a tracker's counters zero); the other slots are
        not touched."""
        m = self._slots_mask(slots)
        self._call('reset', ptr(self._dev_bytes(m)))
        self.hops[m] = 0


class AlignedEchoCanceller:
    """``EchoCanceller`` behind a ``BulkDelay``: process() is aec.process(mic, bulk.process(mic, played, active), ...).  While a slot
    searches the canceller is given zeros to cancel: its residual is the microphone and its weights stay where they are, so nothing
    has to be reset when the lock comes.  Stands wherever an EchoCanceller does (``EchoCancellingEnhancer``,
    ``RateAdaptedEnhancer``)."""
    _BULK = 'delay search'                                 # what the messages call the first stage

    def __init__(self, bulk, aec):
        if bulk.S != aec.S:
            raise ValueError("%s: the %s has %d streams, the canceller %d" % (type(self).__name__, self._BULK, bulk.S, aec.S))
        self.bulk, self.aec, self.S, self.device, self.P = bulk, aec, aec.S, aec.device, aec.P

    def _aligned(self, mic, played, active):
        return self.bulk.process(mic, played, active=active)

    def process(self, mic, played, active=None, adapt=None, want_echo=False, out=None):
        """EchoCanceller.process on `played` delayed by what the search has found (zeros until then)"""
        return self.aec.process(mic, self._aligned(mic, played, active), active=active, adapt=adapt, want_echo=want_echo, out=out)

    def echo_path(self, slots=None):
        """EchoCanceller.echo_path: the path from the ALIGNED `played` to the microphone"""
        return self.aec.echo_path(slots)

    def reset(self, slots):
        """Restart the given slots in both objects: they search again."""
        self.bulk.reset(slots)
        self.aec.reset(slots)
