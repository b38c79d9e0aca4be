"""Residual-echo suppression behind the echo canceller: with near-end noise that never stops, ``EchoCanceller``'s error-regularised step
stays small and some echo stays in its residual.  ``ResidualEchoSuppressor`` is the second stage, a spectral post-filter per stream slot
driven by the canceller's own echo estimate: it removes the part of the residual's power that is coherent with that estimate, so that
the spectrum ``RealtimeEnhancer`` reads as `noise` approaches the noise's.  256-sample hops, sqrt-Hann 512-sample frames, float64
transforms, in libnele_hip.so (csrc/res.hip, the ``nele_res_*`` entry points of include/nele_hip_ext.h; the arithmetic is DESIGN.md
section 17).  This module owns memory and bookkeeping only; there is no arithmetic in torch.

    res = ResidualEchoSuppressor(streams=256)
    clean_residual = res.process(residual_hops, echo_hops)      # [256, nh * 256] each, as EchoCanceller.process(..., want_echo=True)
                                                                # returns them; the output is ONE HOP LATE (a slot's first hop: zeros to rounding)

    aec = SuppressedEchoCanceller(EchoCanceller(256, partitions=8), res)      # or around an AlignedEchoCanceller
    loop = EchoCancellingEnhancer(RealtimeEnhancer(...), aec)                 # as with a bare EchoCanceller

    python -m nele_gan_amd.aec --mic mic.wav --played far.wav --out residual.wav --suppress [--res-beta 2.0] [--res-gmin 0.1]
"""
import numpy as np
import torch

from ._lib import c_longlong, call, lib, ptr, stream
from ._slots import SlotState, dev_rows, host_flags

HOP = 256
NBINS = 257


class ResidualEchoSuppressor(SlotState):
    """B independent suppressors.  beta (>= 0): how much of the coherent power is taken out (2.0 over-subtracts, the smoothed
    cross-spectrum under-estimates it); gmin (0 < gmin <= 1): the floor of the gain, 0.1 = -20 dB."""

    def __init__(self, streams, beta=2.0, gmin=0.1, device='cuda'):
        super().__init__(streams)
        self.beta, self.gmin = float(beta), float(gmin)
        if not (0.0 <= self.beta < float('inf')) or not (0.0 < self.gmin <= 1.0):
            raise ValueError("ResidualEchoSuppressor: needs beta >= 0 and 0 < gmin <= 1 (got %g, %g)" % (self.beta, self.gmin))
        self._alloc(device, lib.nele_res_state_bytes(self.S))
        call('nele_res_init', ptr(self.state), c_longlong(self.nbytes), self.S, stream())

    # ---- streaming
    def process(self, residual, echo, active=None, want_gains=False, out=None):
        """residual, echo [streams, nh * 256] float32 (host, pinned host or device): the canceller's two outputs -> the suppressed
        residual [streams, nh * 256] on the device, one hop late: hop h of the output is hop h - 1 of the input, filtered (with
        want_gains: (suppressed, gains), gains float64 [streams, nh, 257], the gain of every bin and hop).  active: host bool sequence
        [streams] or None (all): inactive slots are neither read nor changed and their output columns are left as they were.  out: a
        buffer, or (buffer, gains buffer), on the device to write into - the way to keep an inactive slot's columns; without it the
        outputs are fresh tensors and an inactive slot's columns undefined.  Never blocks the host."""
        o, g = (out if isinstance(out, (tuple, list)) else (out, None)) if out is not None else (None, None)
        _, nh, e, y, act, flags, o = self._hop_args(residual, echo, ('residual', 'echo'), active, o)
        g = self._out(g, (self.S, nh, NBINS), torch.float64, 'the gains buffer') if want_gains else None
        call('nele_res_hop', ptr(self.state), c_longlong(self.nbytes), self.S, ptr(e), ptr(y), ptr(flags), nh, self.beta, self.gmin, ptr(o), ptr(g),
             stream())
        self._count(act, nh)
        return (o, g) if want_gains else o

    def reset(self, slots):
        """Restart the given slots (zero history, spectra and overlap-add tail); the other slots are not touched."""
        m = self._slots_mask(slots)
        call('nele_res_reset', ptr(self.state), c_longlong(self.nbytes), self.S, ptr(self._dev_bytes(m)), stream())
        self.hops[m] = 0


class SuppressedEchoCanceller:
    """An ``EchoCanceller`` (or ``AlignedEchoCanceller``) with a ``ResidualEchoSuppressor`` behind it: process() is
    res.process(*aec.process(mic, played, ..., want_echo=True), active).  Stands wherever an EchoCanceller does
    (``EchoCancellingEnhancer``, ``RateAdaptedEnhancer``).  What it returns as the residual is ONE HOP LATE against the microphone
    (the suppressor's overlap-add); a noise tracker does not mind.
    A slot's first hop: the suppressor has nothing to give yet (its output there is its zero history), and a noise tracker must not
    start on silence - IMCRA's running minimum of a stream whose first frame is silent stays zero for 120 frames and
    ``RealtimeEnhancer``'s output turns NaN at frame 15.  So in the first hop of a slot's life, and of its life after a reset, this
    class hands on the canceller's own residual of that hop (a copy; the enhancer hears that hop twice, once plain and once
    suppressed)."""

    def __init__(self, aec, res):
        if aec.S != res.S:
            raise ValueError("SuppressedEchoCanceller: the canceller has %d streams, the suppressor %d" % (aec.S, res.S))
        self.aec, self.res, self.S, self.device, self.P = aec, res, aec.S, aec.device, aec.P

    def process(self, mic, played, active=None, adapt=None, want_echo=False, out=None):
        """EchoCanceller.process, the residual suppressed and one hop late (a slot's first hop: see the class); with want_echo:
        (suppressed residual, echo) - the echo is THIS hop's estimate as the canceller gave it, so the two differ by a hop.  out: as
        EchoCanceller.process, a buffer for the suppressed residual or (that, an echo buffer)."""
        o, echo_buf = (out if isinstance(out, (tuple, list)) else (out, None)) if out is not None else (None, None)
        residual, echo = self.aec.process(mic, played, active=active, adapt=adapt, want_echo=True,
                                          out=None if echo_buf is None else (None, echo_buf))
        first = self.res.hops == 0                             # before res.process counts this call's hops
        if active is not None:
            first = first & host_flags(active, self.S, "SuppressedEchoCanceller: active must hold one flag per stream")
        sup = self.res.process(residual, echo, active=active, out=o)
        if first.any():
            rows = dev_rows(np.nonzero(first)[0], sup.device)
            sup[:, :HOP].index_copy_(0, rows, residual[:, :HOP].index_select(0, rows))
        return (sup, echo) if want_echo else sup

    def echo_path(self, slots=None):
        """EchoCanceller.echo_path"""
        return self.aec.echo_path(slots)

    def reset(self, slots):
        """Restart the given slots in both objects."""
        self.aec.reset(slots)
        self.res.reset(slots)
