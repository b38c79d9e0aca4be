"""Clock drift between playback and capture, followed ahead of the echo canceller.  A loudspeaker and a microphone never share a clock:
50 to 200 ppm between them is ordinary, 0.8 to 3.2 samples per second at 16 kHz, and the echo path slides under the canceller all the
time.  ``DriftCompensator`` stands where the bulk search's whole-hop delay line stands: it takes the whole-hop delay from a
``BulkDelay`` or ``TrackingBulkDelay`` on the device, estimates the clock offset from the microphone and its own output, and hands
`played` on delayed by tau(t) samples, tau following the drift.  ``DriftTrackedEchoCanceller`` chains search, compensator and
``EchoCanceller``.  The kernels are in libnele_hip.so (csrc/drift.hip, the ``nele_drift_*`` entry points of include/nele_hip_ext2.h;
the arithmetic is DESIGN.md section 19).  This module owns memory and bookkeeping only; there is no arithmetic in torch.

    search = TrackingBulkDelay(streams=256, blocks=32)
    drift = DriftCompensator(streams=256, blocks=32)
    aligned = drift.process(mic_hops, played_hops, search.delays())      # [256, nh * 256]: zeros until a slot has a base, then `played` late by tau
    drift.status()['drift_ppm']                                          # float64 [256] on the device

    aec = DriftTrackedEchoCanceller(search, drift, EchoCanceller(256, partitions=4))
    loop = EchoCancellingEnhancer(RealtimeEnhancer(...), aec)            # as with a bare EchoCanceller
"""
import numpy as np
import torch

from . import _lib
from ._lib import c_longlong, call, ptr, stream
from ._slots import HOP, SlotState, to_dev

C2 = _lib.CONSTS2
MAX_BLOCKS = _lib.CONSTS['NELE_BULK_MAX_BLOCKS']
MAX_RATE = C2['NELE_DRIFT_MAX_RATE']
INFO = C2['NELE_DRIFT_INFO']
_FIELDS = (('tau', 'NELE_DRIFT_I_TAU'), ('rate', 'NELE_DRIFT_I_RATE'), ('delta', 'NELE_DRIFT_I_DELTA'), ('n', 'NELE_DRIFT_I_N'),
           ('base', 'NELE_DRIFT_I_BASE'), ('snaps', 'NELE_DRIFT_I_SNAPS'))


class DriftCompensator(SlotState):
    """B independent fractional, moving delay lines.  blocks: Q in 2 .. 64, the search's own value (the slot keeps Q + 4 hops of
    `played`); lam_fast < lam_slow in (0, 1): the two averages of the weighted cross-spectrum whose phase slope is the error; kp, ki
    (>= 0): the loop's proportional and integral gains."""

    def __init__(self, streams, blocks=32, lam_fast=0.9, lam_slow=0.99, kp=0.02, ki=5e-4, device='cuda'):
        super().__init__(streams)
        self.Q = int(blocks)
        if not 2 <= self.Q <= MAX_BLOCKS:
            raise ValueError("DriftCompensator: blocks must be in 2 .. %d (got %d)" % (MAX_BLOCKS, self.Q))
        self.lam_fast, self.lam_slow, self.kp, self.ki = float(lam_fast), float(lam_slow), float(kp), float(ki)
        if not (0.0 < self.lam_fast < self.lam_slow < 1.0) or not (0.0 <= self.kp < float('inf')) or not (0.0 <= self.ki < float('inf')):
            raise ValueError("DriftCompensator: needs 0 < lam_fast < lam_slow < 1, kp >= 0 and ki >= 0 (got %g, %g, %g, %g)"
                             % (self.lam_fast, self.lam_slow, self.kp, self.ki))
        self._alloc(device, _lib.lib.nele_drift_state_bytes(self.S, self.Q))
        self._call('init')

    def _call(self, what, *args):
        call('nele_drift_%s' % what, ptr(self.state), c_longlong(self.nbytes), self.S, self.Q, *args, stream())

    # ---- streaming
    def process(self, mic, played, base_hops, active=None, adapt=None, out=None, want_snapped=False):
        """mic, played [streams, nh * 256] float32 (host, pinned host or device), base_hops int32 [streams] ON THE DEVICE (what
        ``BulkDelay.delays()`` / ``TrackingBulkDelay.delays()`` return: hops, -1 = still searching) -> aligned [streams, nh * 256] on
        the device: exact zeros until the slot has taken a base, then `played` late by tau(t) samples.  A base in 0 .. blocks - 1 that
        differs from the one the slot last took snaps it at the first hop of this call (tau = max(256 base, 31), the estimator
        cleared, the rate kept); any other value changes nothing.  active / adapt: host bool sequences [streams] or None (all):
        inactive slots are neither read nor changed and their output columns are left as they were; slots with adapt false warp with
        the tau and rate they have and go on estimating.  out: as in ``BulkDelay.process``.  want_snapped: -> (aligned, snapped),
        snapped uint8 [streams] on the device: 1 for an active slot that snapped in this call, 0 for every other slot.  Never blocks
        the host."""
        if (not isinstance(base_hops, torch.Tensor) or not base_hops.is_cuda or base_hops.dtype != torch.int32
                or tuple(base_hops.shape) != (self.S,)):
            raise ValueError("DriftCompensator.process: base_hops must be int32 [%d] on the device" % self.S)
        _, nh, d, x, act, flags, out = self._hop_args(mic, played, ('mic', 'played'), active, out)
        ada = None if adapt is None else self._dev_bytes(self._flags(adapt, "DriftCompensator: adapt must hold one flag per stream"))
        snapped = torch.empty((self.S,), dtype=torch.uint8, device=self.device) if want_snapped else None
        self._call('hop', ptr(d), ptr(x), ptr(base_hops.contiguous()), ptr(flags), ptr(ada), nh, self.lam_fast, self.lam_slow, self.kp, self.ki,
                   ptr(out), ptr(snapped))
        self._count(act, nh)
        return (out, snapped) if want_snapped else out

    def status(self):
        """-> dict of float64 [streams] device tensors: 'tau' (samples), 'rate' (samples of delay per sample), 'drift_ppm' (-1e6 rate:
        how fast the capture clock runs), 'delta' (the last hop's error, samples), 'n' (hops the estimator has seen since the last
        snap), 'base' (hops, -1 = none taken yet), 'snaps'."""
        info = torch.empty((self.S, INFO), dtype=torch.float64, device=self.device)
        self._call('status', ptr(info))
        st = {name: info[:, C2[const]].contiguous() for name, const in _FIELDS}
        st['drift_ppm'] = st['rate'] * -1e6
        return st

    def set_rate(self, slots, ppm):
        """Start the given slots from a drift the integrator knows: ppm (how fast the capture clock runs), one value for all of them or
        one per slot, within +-1000."""
        slots = np.asarray(slots, dtype=np.int64).reshape(-1)
        v = np.broadcast_to(np.asarray(ppm, dtype=np.float64).reshape(-1), slots.shape) if np.size(ppm) in (1, slots.size) else None
        if v is None or not (np.abs(v) <= MAX_RATE * 1e6).all():
            raise ValueError("DriftCompensator.set_rate: ppm must be one value, or one per slot, within +-%g" % (MAX_RATE * 1e6))
        m = self._slots_mask(slots)
        full = np.zeros(self.S, dtype=np.float64)
        full[slots] = np.clip(-1e-6 * v, -MAX_RATE, MAX_RATE)
        flags, rates = self._dev_bytes(m), to_dev(torch.from_numpy(full), self.device)      # both alive until the call has been enqueued
        self._call('set_rate', ptr(flags), ptr(rates))

    def reset(self, slots):
        """Restart the given slots (an empty ring, no base, rate 0); the other slots are not touched."""
        m = self._slots_mask(slots)
        self._call('reset', ptr(self._dev_bytes(m)))
        self.hops[m] = 0

    def taps(self):
        """-> float64 [65, 64] on the device: the fractional-delay table as the state holds it"""
        t = torch.empty((C2['NELE_DRIFT_PHASES'] + 1, C2['NELE_DRIFT_TAPS']), dtype=torch.float64, device=self.device)
        self._call('taps', ptr(t))
        return t


class DriftTrackedEchoCanceller:
    """``EchoCanceller`` behind a ``DriftCompensator`` behind a ``BulkDelay`` or ``TrackingBulkDelay`` of the same streams and blocks.
    process() runs, in order: the search (its own `aligned` is not used); drift.process(mic, played, search.delays(), ...,
    want_snapped=True); aec.reset_flagged(snapped); aec.process(mic, aligned, ...).  No value is read back to the host.  The
    canceller restarts at the first hop of the call in which a snap fell, so - as with ``TrackedEchoCanceller`` - the composite's bits
    depend on how the hops around a snap are grouped into calls; the compensator's own bits do not, given the same base_hops on every
    call.  (The canceller's host counter ``hops`` is not told of such a restart.)  Stands wherever an EchoCanceller does
    (``EchoCancellingEnhancer``, ``SuppressedEchoCanceller``, ``RateAdaptedEnhancer``)."""

    def __init__(self, search, drift, aec):
        if not (search.S == drift.S == aec.S):
            raise ValueError("DriftTrackedEchoCanceller: the delay search has %d streams, the compensator %d, the canceller %d"
                             % (search.S, drift.S, aec.S))
        if search.Q != drift.Q:
            raise ValueError("DriftTrackedEchoCanceller: the delay search has blocks=%d, the compensator blocks=%d" % (search.Q, drift.Q))
        self.search, self.drift, self.aec, self.S, self.device, self.P = search, drift, aec, aec.S, aec.device, aec.P

    def process(self, mic, played, active=None, adapt=None, want_echo=False, out=None):
        """EchoCanceller.process on `played` delayed by what the search and the compensator hold (zeros until the search has locked)"""
        self.search.process(mic, played, active=active)
        aligned, snapped = self.drift.process(mic, played, self.search.delays(), active=active, want_snapped=True)
        self.aec.reset_flagged(snapped)
        return self.aec.process(mic, aligned, active=active, adapt=adapt, want_echo=want_echo, out=out)

    def echo_path(self, slots=None):
        """EchoCanceller.echo_path: the path from the ALIGNED `played` to the microphone"""
        return self.aec.echo_path(slots)

    def reset(self, slots):
        """Restart the given slots in all three objects: they search again."""
        self.search.reset(slots)
        self.drift.reset(slots)
        self.aec.reset(slots)
