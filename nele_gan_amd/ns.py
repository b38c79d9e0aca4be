"""Noise suppression for the uplink of the real-time path: what ``EchoCanceller`` leaves of the microphone signal is the near-end talker
plus the room's noise, and in a two-way call that residual is what the far end hears.  ``NoiseSuppressor`` takes the noise out of it,
per stream slot: the optimally-modified log-spectral amplitude gain (Cohen & Berdugo 2001) on the project's IMCRA noise tracker,
256-sample hops, sqrt-Hann 512-sample frames, float64 transforms, in libnele_hip.so (csrc/ns.hip, the ``nele_ns_*`` entry points of
include/nele_hip_ext4.h; the arithmetic is DESIGN.md section 21).  This module owns memory and bookkeeping only; there is no arithmetic
in torch.

    ns = NoiseSuppressor(streams=256)
    uplink = ns.process(residual_hops)                          # [256, nh * 256] -> the same shape, ONE HOP LATE
    uplink, gains, psd = ns.process(residual_hops, want=('gains', 'noise_psd'))     # float64 [256, nh, 257] each

    duplex = DuplexEnhancer(EchoCancellingEnhancer(RealtimeEnhancer(...), EchoCanceller(256)), ns)
    out, uplink = duplex.process(clean_hops, mic_hops)          # out: what the loudspeaker plays; uplink: what the far end hears

    python -m nele_gan_amd.ns --in noisy.wav --out suppressed.wav [--gmin 0.1]
    python -m nele_gan_amd.aec --mic mic.wav --played far.wav --out residual.wav --uplink uplink.wav [--uplink-gmin 0.1]
"""
import numpy as np
import torch

from ._lib import c_longlong, call, lib, ptr, stream
from ._slots import SlotState

HOP = 256
NBINS = 257
WANT = ('gains', 'noise_psd', 'presence')


class NoiseSuppressor(SlotState):
    """B independent suppressors.  gmin (0 < gmin <= 1): the gain of a bin without speech, 0.1 = -20 dB.
    The first 15 frames of a slot's life, and of its life after a reset (240 ms), come out at gmin in every bin: IMCRA takes them as
    noise to start its estimate on."""

    def __init__(self, streams, gmin=0.1, device='cuda'):
        super().__init__(streams)
        self.gmin = float(gmin)
        if not (0.0 < self.gmin <= 1.0):
            raise ValueError("NoiseSuppressor: needs 0 < gmin <= 1 (got %g)" % self.gmin)
        self._alloc(device, lib.nele_ns_state_bytes(self.S))
        call('nele_ns_init', ptr(self.state), c_longlong(self.nbytes), self.S, stream())

    # ---- streaming
    def process(self, x, active=None, want=(), out=None):
        """x [streams, nh * 256] float32 (host, pinned host or device): the canceller's residual -> the suppressed signal
        [streams, nh * 256] on the device, one hop late: hop h of the output is hop h - 1 of the input, filtered.  want: any of
        'gains', 'noise_psd', 'presence' - the call then returns a tuple, the output followed by those in the order asked for, each
        float64 [streams, nh, 257]: the gain, the noise PSD estimate after the frame, and the speech-presence probability of every bin
        and hop.  active: host bool sequence [streams] or None (all): inactive slots are neither read nor changed and their output
        columns are left as they were.  out: a buffer, or (buffer, one buffer per name in want), on the device to write into - the
        way to keep an inactive slot's columns; without it the outputs are fresh tensors and an inactive slot's columns undefined.
        Never blocks the host."""
        want = (want,) if isinstance(want, str) else tuple(want)
        if [n for n in want if n not in WANT] or len(set(want)) != len(want):
            raise ValueError("NoiseSuppressor.process: want must be distinct names out of %s (got %s)" % (WANT, want))
        bufs = list(out) if isinstance(out, (tuple, list)) else [out]
        if len(bufs) not in (1, 1 + len(want)):
            raise ValueError("NoiseSuppressor.process: out must be a buffer or (buffer, one per name in want)")
        bufs += [None] * (1 + len(want) - len(bufs))
        shape = tuple(np.shape(x))
        if len(shape) != 2 or shape[0] != self.S or shape[1] % HOP or shape[1] == 0:
            raise ValueError("NoiseSuppressor.process: x must be [%d, nh * 256]" % self.S)
        nh, xd = shape[1] // HOP, self._dev_f32(x, shape, 'x')
        act = None if active is None else self._flags(active, "NoiseSuppressor: active must hold one flag per stream")
        flags = None if act is None else self._dev_bytes(act)
        o = self._out(bufs[0], shape)
        extra = {n: self._out(bufs[1 + i], (self.S, nh, NBINS), torch.float64, 'the %s buffer' % n) for i, n in enumerate(want)}
        call('nele_ns_hop', ptr(self.state), c_longlong(self.nbytes), self.S, ptr(xd), ptr(flags), nh, self.gmin, ptr(o),
             ptr(extra.get('gains')), ptr(extra.get('noise_psd')), ptr(extra.get('presence')), stream())
        self._count(act, nh)
        return (o,) + tuple(extra[n] for n in want) if want else o

    def reset(self, slots):
        """Restart the given slots (zero history, overlap-add tail and tracker: the next 15 frames are taken as noise again); the other
        slots are not touched."""
        m = self._slots_mask(slots)
        call('nele_ns_reset', ptr(self.state), c_longlong(self.nbytes), self.S, ptr(self._dev_bytes(m)), stream())
        self.hops[m] = 0


class DuplexEnhancer:
    """Both directions of a call: an ``EchoCancellingEnhancer`` for the listener and a ``NoiseSuppressor`` on its canceller's residual
    for the far end.  Per call
        out, residual = loop.process(clean, mic, want_residual=True);  uplink = ns.process(residual)
    `out` is what loop.process alone returns, bit for bit.  The uplink is one hop late against the microphone (the suppressor's
    overlap-add); behind a ``SuppressedEchoCanceller`` the residual already is one hop late, so the uplink is TWO hops late.  Works
    around any canceller the loop accepts."""

    def __init__(self, loop, ns):
        if loop.S != ns.S:
            raise ValueError("DuplexEnhancer: the loop has %d streams, the suppressor %d" % (loop.S, ns.S))
        self.loop, self.ns, self.S = loop, ns, loop.S

    def process(self, clean, mic, active=None):
        """clean, mic [streams, nh * 256] float32 -> (out, uplink), [streams, nh * 256] each; active as EchoCancellingEnhancer's: an
        inactive slot's columns of both are undefined."""
        out, residual = self.loop.process(clean, mic, active=active, want_residual=True)
        return out, self.ns.process(residual, active=active)

    def finish(self, slots, clean_tail, mic_tail, tail_lengths, debug=None):
        """EchoCancellingEnhancer.finish; the suppressor's last half frame is not flushed."""
        return self.loop.finish(slots, clean_tail, mic_tail, tail_lengths, debug=debug)

    def reset(self, slots):
        """Restart the given slots in both objects."""
        self.loop.reset(slots)
        self.ns.reset(slots)


# ------------------------------------------------------------------------------------------------------------------ command line
def suppress_file(x, gmin=0.1, device='cuda'):
    """x: float32 array of length L -> the suppressed signal [L] float32, one hop late as process() returns it: the whole hops through one
    NoiseSuppressor call, the last L % 256 samples zero-padded to one more hop and cut again; the file's last hop does not come out."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    if x.size == 0:
        raise ValueError("ns: the input is empty")
    L = x.size
    nh = (L + HOP - 1) // HOP
    d = np.zeros((1, nh * HOP), dtype=np.float32)
    d[0, :L] = x
    return NoiseSuppressor(1, gmin=gmin, device=device).process(torch.from_numpy(d))[0, :L].cpu().numpy()


def build_parser():
    import argparse
    ap = argparse.ArgumentParser(prog='python -m nele_gan_amd.ns', description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--in', dest='inp', required=True, help='16 kHz PCM_16 wav: speech in noise (the echo canceller\'s residual)')
    ap.add_argument('--out', required=True, help='the noise-suppressed signal, PCM_16, one 256-sample hop late')
    ap.add_argument('--gmin', type=float, default=0.1, help='the gain of a bin without speech, in (0, 1]')
    return ap


def main(argv=None):
    from . import dataio
    ap = build_parser()
    a = ap.parse_args(argv)
    if not (0.0 < a.gmin <= 1.0):
        ap.error('needs 0 < --gmin <= 1')
    wav, sr = dataio.read_wav(a.inp)
    if sr != dataio.fs:
        ap.error('%s is sampled at %d Hz, not %d: convert it first with python -m nele_gan_amd.resample' % (a.inp, sr, dataio.fs))
    if len(wav) == 0:
        ap.error('%s is empty' % a.inp)
    out = suppress_file(wav, gmin=a.gmin)
    dataio.write_wav_pcm16(a.out, out)
    print('%s: %d samples, noise suppressed (gmin %g): the output is one hop (%d ms) late' % (a.out, len(out), a.gmin, HOP * 1000 // dataio.fs))
    return 0


if __name__ == '__main__':
    import sys
    sys.exit(main())
