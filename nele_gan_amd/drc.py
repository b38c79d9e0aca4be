"""Dynamic range compression behind the enhancer of the real-time path: the other half of SSDRC (Zorila, Kandia & Stylianou 2012), whose
compressor the project otherwise has only as an offline, whole-utterance stage (``ssdrc.ssdrc_compress``).
``StreamCompressor`` is its causal form, per stream slot: 256-sample hops, the Hilbert envelope with 144 samples of look-ahead, the
attack / release recursion, the static curve against e0_ratio times a decaying maximum of the envelope (time constant tau_peak) and an
equaliser that holds the output's recursive energy (time constant tau_energy) at the input's - in libnele_hip.so (csrc/drc.hip, the
``nele_drc_*`` entry points of include/nele_hip_ext6.h; the arithmetic is DESIGN.md section 23).  This module owns memory and
bookkeeping only; there is no arithmetic in torch.

    drc = StreamCompressor(streams=256)
    out = drc.process(hops)                                     # [256, nh * 256] -> the same shape, ONE HOP LATE
    out, gain, level = drc.process(hops, want=('gain', 'level'))    # float64 [256, nh * 256] and [256, nh]

    chain = CompressedEnhancer(RealtimeEnhancer(rule=SiiOptRule(), streams=256), drc)
    out = chain.process(clean_hops, noise_hops)                 # what the loudspeaker plays, two hops behind `clean_hops`
    loop = EchoCancellingEnhancer(chain, EchoCanceller(256))    # the chain stands where a RealtimeEnhancer does

    python -m nele_gan_amd.drc --in speech.wav --out compressed.wav [--tau-peak 4 --tau-energy 1 --no-equalise]

THE ECHO LOOP MUST SEE THE COMPRESSED SIGNAL.  The canceller's reference is what the loudspeaker plays.  Compress inside the loop -
``EchoCancellingEnhancer(CompressedEnhancer(rt, drc), aec)``, whose ``played`` is then the compressor's output - and never behind it:
a compressor between ``EchoCancellingEnhancer.process`` and the loudspeaker is a time-varying gain in the echo path that the
canceller has to chase, and its one hop of delay moves the echo.
"""
import ctypes
import math

import numpy as np
import torch

from ._lib import c_longlong, call, lib, ptr, stream
from ._slots import SlotState, dev_rows, to_dev
from .ssdrc import SsdrcParams

HOP = 256
WANT = ('gain', 'level')


def hop_factor(tau, name):
    """a time constant in seconds -> the per-hop forgetting factor exp(-0.016 / tau), in float64"""
    tau = float(tau)
    if not (tau > 0.0 and math.isfinite(tau)):
        raise ValueError("StreamCompressor: %s must be a positive number of seconds (got %r)" % (name, tau))
    f = float(np.exp(-0.016 / tau))
    if not f < 1.0:
        raise ValueError("StreamCompressor: %s=%g s is too long: its per-hop factor rounds to 1" % (name, tau))
    return f


class StreamCompressor(SlotState):
    """B independent compressors.  params: an ``ssdrc.SsdrcParams`` - attack, release, e0_ratio and knots are used, with section 11's
    defaults.  tau_peak, tau_energy [s]: the time constants of the envelope maximum the reference level follows and of the equaliser's
    two energies.  equalise=False: the compressed signal as it is.  ref_level: None, or one fixed reference level e0 >= 0 per stream
    in the envelope's units (0: that stream passes through) - then the decaying maximum is tracked but not used.
    A NaN sample stays in a slot's envelope until the slot is reset."""

    def __init__(self, streams, params=None, tau_peak=4.0, tau_energy=1.0, equalise=True, ref_level=None, device='cuda'):
        super().__init__(streams)
        self.params = params if params is not None else SsdrcParams()
        if not isinstance(self.params, SsdrcParams):
            raise ValueError("StreamCompressor: params must be an ssdrc.SsdrcParams")
        p = self.params
        if not (0.0 <= p.attack < 1.0 and 0.0 <= p.release < 1.0):
            raise ValueError("StreamCompressor: attack / release outside [0, 1)")
        if not (p.e0_ratio > 0.0 and math.isfinite(p.e0_ratio)):
            raise ValueError("StreamCompressor: e0_ratio must be positive and finite")
        kx = [float(k[0]) for k in p.knots]
        if not all(math.isfinite(v) for k in p.knots for v in k) or any(a >= b for a, b in zip(kx, kx[1:])):
            raise ValueError("StreamCompressor: knots must be finite with ascending inputs")
        self._c = p.c_struct()                             # (raises unless 2 .. 8 knots)
        self.rho, self.lam = hop_factor(tau_peak, 'tau_peak'), hop_factor(tau_energy, 'tau_energy')
        self.equalise = bool(equalise)
        lv = None
        if ref_level is not None:
            lv = np.asarray(ref_level, dtype=np.float64).reshape(-1)
            if lv.shape[0] != self.S or not np.all(np.isfinite(lv)) or np.any(lv < 0):
                raise ValueError("StreamCompressor: ref_level must hold one finite level >= 0 per stream (%d)" % self.S)
        self._alloc(device, lib.nele_drc_state_bytes(self.S))
        self.ref_level = None if lv is None else to_dev(torch.from_numpy(lv.copy()), self.device)
        call('nele_drc_init', ptr(self.state), c_longlong(self.nbytes), self.S, stream())

    # ---- streaming
    def process(self, x, active=None, want=(), out=None):
        """x [streams, nh * 256] float32 (host, pinned host or device) -> the compressed signal [streams, nh * 256] on the device, one
        hop late: hop h of the output is hop h - 1 of the input, compressed; a slot's first hop yields zeros.  want: any of 'gain',
        'level' - the call then returns a tuple, the output followed by those in the order asked for: the total gain on every output
        sample, float64 [streams, nh * 256], and the reference level e0 of every hop, float64 [streams, nh] (both 0 in a slot's first
        hop).  active: host bool sequence [streams] or None (all): inactive slots are neither read nor changed and their output
        columns are left as they were.  out: a buffer, or (buffer, one buffer per name in want), on the device to write into - the
        way to keep an inactive slot's columns; without it the outputs are fresh tensors and an inactive slot's columns undefined.
        Never blocks the host."""
        want = (want,) if isinstance(want, str) else tuple(want)
        if [n for n in want if n not in WANT] or len(set(want)) != len(want):
            raise ValueError("StreamCompressor.process: want must be distinct names out of %s (got %s)" % (WANT, want))
        bufs = list(out) if isinstance(out, (tuple, list)) else [out]
        if len(bufs) not in (1, 1 + len(want)):
            raise ValueError("StreamCompressor.process: out must be a buffer or (buffer, one per name in want)")
        bufs += [None] * (1 + len(want) - len(bufs))
        shape = tuple(np.shape(x))
        if len(shape) != 2 or shape[0] != self.S or shape[1] % HOP or shape[1] == 0:
            raise ValueError("StreamCompressor.process: x must be [%d, nh * 256]" % self.S)
        nh, xd = shape[1] // HOP, self._dev_f32(x, shape, 'x')
        act = None if active is None else self._flags(active, "StreamCompressor: active must hold one flag per stream")
        flags = None if act is None else self._dev_bytes(act)
        o = self._out(bufs[0], shape)
        shapes = {'gain': shape, 'level': (self.S, nh)}
        extra = {n: self._out(bufs[1 + i], shapes[n], torch.float64, 'the %s buffer' % n) for i, n in enumerate(want)}
        call('nele_drc_hop', ptr(self.state), c_longlong(self.nbytes), self.S, ptr(xd), ptr(flags), nh, ctypes.byref(self._c), self.rho,
             self.lam, int(self.equalise), ptr(self.ref_level), ptr(o), ptr(extra.get('gain')), ptr(extra.get('level')), stream())
        self._count(act, nh)
        return (o,) + tuple(extra[n] for n in want) if want else o

    def reset(self, slots):
        """Restart the given slots (zero history, envelope, maximum and energies); the other slots are not touched."""
        m = self._slots_mask(slots)
        call('nele_drc_reset', ptr(self.state), c_longlong(self.nbytes), self.S, ptr(self._dev_bytes(m)), stream())
        self.hops[m] = 0


class CompressedEnhancer:
    """A ``RealtimeEnhancer`` with a ``StreamCompressor`` behind it: per call  out = drc.process(rt.process(clean, noise)).  It stands
    where a ``RealtimeEnhancer`` does - inside ``EchoCancellingEnhancer`` too, whose ``played`` is then the compressed signal (see the
    module's docstring).  The output is one hop later than the enhancer's own, two hops behind the input."""

    def __init__(self, rt, drc):
        if rt.S != drc.S:
            raise ValueError("CompressedEnhancer: the enhancer has %d streams, the compressor %d" % (rt.S, drc.S))
        self.rt, self.drc, self.S = rt, drc, rt.S

    def process(self, clean, noise, active=None, debug=None):
        """RealtimeEnhancer.process, compressed; an inactive slot's columns are undefined."""
        kw = {} if debug is None else {'debug': debug}
        return self.drc.process(self.rt.process(clean, noise, active=active, **kw), active=active)

    def finish(self, slots, clean_tail, noise_tail, tail_lengths, debug=None):
        """End the streams of ``slots``: RealtimeEnhancer.finish, then its hop and one zero hop through the compressor on those slots
        -> [len(slots), 512], the two hops this emits: the enhancer's last whole hop and its finishing hop, compressed - the stream's
        last samples."""
        slots = np.asarray(slots, dtype=np.int64).reshape(-1)
        kw = {} if debug is None else {'debug': debug}
        last = self.rt.finish(slots, clean_tail, noise_tail, tail_lengths, **kw)
        rows = dev_rows(slots, last.device)
        full = torch.zeros((self.S, 2 * HOP), dtype=torch.float32, device=last.device)
        full[:, :HOP].index_copy_(0, rows, last)
        act = np.zeros(self.S, dtype=bool)
        act[slots] = True
        return self.drc.process(full, active=act).index_select(0, rows)

    def reset(self, slots):
        """Restart the given slots in both objects."""
        self.rt.reset(slots)
        self.drc.reset(slots)


# ------------------------------------------------------------------------------------------------------------------ command line
def compress_file(x, tau_peak=4.0, tau_energy=1.0, equalise=True, params=None, device='cuda'):
    """x: float32 array of length L -> the compressed signal [L] float32, realigned: the whole hops and the zero-padded tail through
    one StreamCompressor call together with one zero hop that flushes the last one."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    if x.size == 0:
        raise ValueError("drc: the input is empty")
    L = x.size
    nh = (L + HOP - 1) // HOP
    d = np.zeros((1, (nh + 1) * HOP), dtype=np.float32)
    d[0, :L] = x
    drc = StreamCompressor(1, params=params, tau_peak=tau_peak, tau_energy=tau_energy, equalise=equalise, device=device)
    return drc.process(torch.from_numpy(d))[0, HOP:HOP + L].cpu().numpy()


def build_parser():
    import argparse
    ap = argparse.ArgumentParser(prog='python -m nele_gan_amd.drc', description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--in', dest='inp', required=True, help='16 kHz PCM_16 wav: what the enhancer made, or plain speech')
    ap.add_argument('--out', required=True, help='the compressed signal, PCM_16, aligned with the input')
    ap.add_argument('--tau-peak', type=float, default=4.0, help='time constant [s] of the envelope maximum the reference level follows')
    ap.add_argument('--tau-energy', type=float, default=1.0, help='time constant [s] of the equaliser\'s energies')
    ap.add_argument('--no-equalise', action='store_true', help='switch the energy equaliser off')
    return ap


def main(argv=None):
    from . import dataio
    ap = build_parser()
    a = ap.parse_args(argv)
    for flag, tau in (('--tau-peak', a.tau_peak), ('--tau-energy', a.tau_energy)):
        try:
            hop_factor(tau, flag)
        except ValueError:
            ap.error('%s must be a positive number of seconds (not so long that exp(-0.016 / tau) rounds to 1)' % flag)
    wav, sr = dataio.read_wav(a.inp)
    if sr != dataio.fs:
        ap.error('%s is sampled at %d Hz, not %d: convert it first with python -m nele_gan_amd.resample' % (a.inp, sr, dataio.fs))
    if len(wav) == 0:
        ap.error('%s is empty' % a.inp)
    out = compress_file(wav, tau_peak=a.tau_peak, tau_energy=a.tau_energy, equalise=not a.no_equalise)
    clipped = int(np.sum(np.abs(out) * np.float32(32767.0) > 32767.5))
    dataio.write_wav_pcm16(a.out, out)
    print('%s: %d samples, compressed (tau_peak %g s, tau_energy %g s, equaliser %s): %d clipped samples saturated'
          % (a.out, len(out), a.tau_peak, a.tau_energy, 'off' if a.no_equalise else 'on', clipped))
    return 0


if __name__ == '__main__':
    import sys
    sys.exit(main())
