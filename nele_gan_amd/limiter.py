"""A look-ahead true-peak limiter as the last stage of the real-time path: nothing else in the chain bounds the peak of what the
loudspeaker plays - ``RealtimeEnhancer`` applies no final gain, the SII rule raises the crest factor, ``StreamCompressor`` shapes the
envelope but guarantees no peak.  ``StreamLimiter`` does, per stream slot: 256-sample hops at 16 kHz, one hop late, a peak detector
that also looks at the three quarter points between samples, `lookahead` samples over which the gain ramps into a peak, an
exponential release - in libnele_hip.so (csrc/limiter.hip, the ``nele_lim_*`` entry points of include/nele_hip_ext9.h; the arithmetic
is DESIGN.md section 26).  Its claim is peak control without harmonic distortion, not a higher SIIB than clipping (section 26's
table).  This module owns memory and bookkeeping only; there is no arithmetic in torch.

    lim = StreamLimiter(streams=256, ceiling_db=-1.0)
    out = lim.process(hops)                                     # [256, nh * 256] -> the same shape, ONE HOP LATE, |out| <= ceiling
    out, gain, peak = lim.process(hops, want=('gain', 'peak'))  # float64 [256, nh * 256] and [256, nh]

    chain = LimitedEnhancer(CompressedEnhancer(RealtimeEnhancer(rule=SiiOptRule(), streams=256), StreamCompressor(256)), lim)
    out = chain.process(clean_hops, noise_hops)                 # what the loudspeaker plays, three hops behind `clean_hops`
    loop = EchoCancellingEnhancer(chain, EchoCanceller(256))    # the chain stands where a RealtimeEnhancer does

    python -m nele_gan_amd.limiter --in speech.wav --out limited.wav [--ceiling-db -1 --drive-db 0 --lookahead-ms 5 --release-ms 100 --sample-peak]

THE ECHO LOOP MUST SEE THE LIMITED SIGNAL.  The canceller's reference is what the loudspeaker plays.  Limit inside the loop -
``EchoCancellingEnhancer(LimitedEnhancer(inner, lim), aec)``, whose ``played`` is then the limiter's output - and never behind it: a
limiter, a saturating DAC or a PCM_16 writer between ``EchoCancellingEnhancer.process`` and the loudspeaker is a nonlinearity in the
echo path, which the canceller cannot model, and the limiter's one hop of delay moves the echo.

Behind ``streamrate.adapt(..., highband=True)`` the band above 8 kHz is carried past the whole 16 kHz chain and added BEHIND the
limiter: it is not limited, and the up-converter reconstructs peaks between the 16 kHz samples that the 4 x detector holds to within
about 1 % of the ceiling (section 26).  A limiter at the device rate is not part of this module.
"""
import ctypes
import math

import numpy as np
import torch

from ._lib import CONSTS9, c_longlong, call, lib, ptr, stream
from ._slots import SlotState, dev_rows

HOP = CONSTS9['NELE_LIM_HOP']
MAX_LOOKAHEAD = CONSTS9['NELE_LIM_MAX_LOOKAHEAD']
WANT = ('gain', 'peak')
FS = 16000


def true_peak_taps():
    """float64 [3, 12]: tap k (k = 1, 2, 3) at offset m = -5 .. 6 is sinc(m - k / 4) (0.5 + 0.5 cos(pi (m - k / 4) / 6)) - the
    Hann-windowed interpolators of the three quarter points between a sample and the next"""
    m = np.arange(-5, 7, dtype=np.float64)
    t = np.stack([m - k / 4.0 for k in (1, 2, 3)])
    return np.sinc(t) * (0.5 + 0.5 * np.cos(np.pi * t / 6.0))


def db_factor(db, name):
    """dB -> the linear factor 10^(db / 20) in float64, which must be positive and finite"""
    db = float(db)
    with np.errstate(over='ignore'):
        f = float(np.float64(10.0) ** (db / 20.0)) if math.isfinite(db) else 0.0
    if not (f > 0.0 and math.isfinite(f)):
        raise ValueError("StreamLimiter: %s=%r leaves no positive finite factor" % (name, db))
    return f


def release_factor(seconds):
    """a release time in seconds -> the per-sample factor exp(-1 / (16000 seconds)) in float64; 0 s is 0: no hold"""
    seconds = float(seconds)
    if not (seconds >= 0.0 and math.isfinite(seconds)):
        raise ValueError("StreamLimiter: release must be a number of seconds >= 0 (got %r)" % seconds)
    f = 0.0 if seconds == 0.0 else float(np.exp(-1.0 / (FS * seconds)))
    if not f < 1.0:
        raise ValueError("StreamLimiter: release=%g s is too long: its per-sample factor rounds to 1" % seconds)
    return f


class StreamLimiter(SlotState):
    """B independent limiters.  ceiling_db: the ceiling in dBFS (any finite value).  drive_db: a fixed gain in front of the limiter.
    lookahead: samples, 1 .. 192, over which the gain ramps into a peak (80 = 5 ms).  release [s]: the time constant with which the
    reduction decays.  true_peak=False: the detector looks at the samples only.  A NaN sample does not reach the state: it asks for no
    reduction and leaves through the output, at most 6 samples wide."""

    def __init__(self, streams, ceiling_db=-1.0, drive_db=0.0, lookahead=80, release=0.1, true_peak=True, device='cuda'):
        super().__init__(streams)
        self.ceiling, self.drive = db_factor(ceiling_db, 'ceiling_db'), db_factor(drive_db, 'drive_db')
        if int(lookahead) != lookahead or not 1 <= int(lookahead) <= MAX_LOOKAHEAD:
            raise ValueError("StreamLimiter: lookahead must be a whole number of samples in 1 .. %d (got %r)" % (MAX_LOOKAHEAD, lookahead))
        self.lookahead = int(lookahead)
        self.rel = release_factor(release)
        self.taps = true_peak_taps() if true_peak else None
        self._taps = None if self.taps is None else (ctypes.c_double * CONSTS9['NELE_LIM_TAPS'])(*self.taps.reshape(-1))
        self._alloc(device, lib.nele_lim_state_bytes(self.S, self.lookahead))
        call('nele_lim_init', ptr(self.state), c_longlong(self.nbytes), self.S, self.lookahead, stream())

    # ---- streaming
    def process(self, x, active=None, want=(), out=None):
        """x [streams, nh * 256] float32 (host, pinned host or device) -> the limited signal [streams, nh * 256] on the device, one hop
        late: hop h of the output is hop h - 1 of the input, limited; a slot's first hop yields zeros.  want: any of 'gain', 'peak' -
        the call then returns a tuple, the output followed by those in the order asked for: the gain on every output sample, float64
        [streams, nh * 256], and the largest detected peak of every emitted hop, float64 [streams, nh] (both 0 in a slot's first hop).
        active: host bool sequence [streams] or None (all): inactive slots are neither read nor changed and their output columns are
        left as they were.  out: a buffer, or (buffer, one buffer per name in want), on the device to write into - the way to keep an
        inactive slot's columns; without it the outputs are fresh tensors and an inactive slot's columns undefined.
        Never blocks the host."""
        want = (want,) if isinstance(want, str) else tuple(want)
        if [n for n in want if n not in WANT] or len(set(want)) != len(want):
            raise ValueError("StreamLimiter.process: want must be distinct names out of %s (got %s)" % (WANT, want))
        bufs = list(out) if isinstance(out, (tuple, list)) else [out]
        if len(bufs) not in (1, 1 + len(want)):
            raise ValueError("StreamLimiter.process: out must be a buffer or (buffer, one per name in want)")
        bufs += [None] * (1 + len(want) - len(bufs))
        shape = tuple(np.shape(x))
        if len(shape) != 2 or shape[0] != self.S or shape[1] % HOP or shape[1] == 0:
            raise ValueError("StreamLimiter.process: x must be [%d, nh * 256]" % self.S)
        nh, xd = shape[1] // HOP, self._dev_f32(x, shape, 'x')
        act = None if active is None else self._flags(active, "StreamLimiter: active must hold one flag per stream")
        flags = None if act is None else self._dev_bytes(act)
        o = self._out(bufs[0], shape)
        shapes = {'gain': shape, 'peak': (self.S, nh)}
        extra = {n: self._out(bufs[1 + i], shapes[n], torch.float64, 'the %s buffer' % n) for i, n in enumerate(want)}
        call('nele_lim_hop', ptr(self.state), c_longlong(self.nbytes), self.S, ptr(xd), ptr(flags), nh, self.ceiling, self.drive,
             self.lookahead, self.rel, self._taps, ptr(o), ptr(extra.get('gain')), ptr(extra.get('peak')), stream())
        self._count(act, nh)
        return (o,) + tuple(extra[n] for n in want) if want else o

    def reset(self, slots):
        """Restart the given slots (zero history, no reduction); the other slots are not touched."""
        m = self._slots_mask(slots)
        call('nele_lim_reset', ptr(self.state), c_longlong(self.nbytes), self.S, self.lookahead, ptr(self._dev_bytes(m)), stream())
        self.hops[m] = 0


class LimitedEnhancer:
    """A ``RealtimeEnhancer`` or a ``CompressedEnhancer`` with a ``StreamLimiter`` behind it: per call
    out = lim.process(inner.process(clean, noise)).  It stands where a ``RealtimeEnhancer`` does - inside ``EchoCancellingEnhancer``
    too, whose ``played`` is then the limited signal (see the module's docstring).  ``lag_hops``: the hops the output is behind the
    input, the inner object's and the limiter's one - 2 around a RealtimeEnhancer, 3 around a CompressedEnhancer."""

    def __init__(self, inner, lim):
        if inner.S != lim.S:
            raise ValueError("LimitedEnhancer: the enhancer has %d streams, the limiter %d" % (inner.S, lim.S))
        self.inner, self.lim, self.S = inner, lim, inner.S
        self.lag_hops = getattr(inner, 'lag_hops', 2 if hasattr(inner, 'drc') else 1) + 1

    @property
    def device(self):
        return self.lim.device

    def process(self, clean, noise, active=None, debug=None):
        """the inner object's process, limited; an inactive slot's columns are undefined."""
        kw = {} if debug is None else {'debug': debug}
        return self.lim.process(self.inner.process(clean, noise, active=active, **kw), active=active)

    def finish(self, slots, clean_tail, noise_tail, tail_lengths, debug=None):
        """End the streams of ``slots``: the inner object's finish, then its hops and one zero hop through the limiter on those slots
        -> [len(slots), 256 (k + 1)] for the k hops the inner finish returns: one hop more, the stream's last samples, limited."""
        slots = np.asarray(slots, dtype=np.int64).reshape(-1)
        kw = {} if debug is None else {'debug': debug}
        last = self.inner.finish(slots, clean_tail, noise_tail, tail_lengths, **kw)
        rows = dev_rows(slots, last.device)
        full = torch.zeros((self.S, last.shape[1] + HOP), dtype=torch.float32, device=last.device)
        full[:, :last.shape[1]].index_copy_(0, rows, last)
        act = np.zeros(self.S, dtype=bool)
        act[slots] = True
        return self.lim.process(full, active=act).index_select(0, rows)

    def reset(self, slots):
        """Restart the given slots in both objects."""
        self.inner.reset(slots)
        self.lim.reset(slots)


# ------------------------------------------------------------------------------------------------------------------ command line
def limit_file(x, device='cuda', **kw):
    """x: float32 array of length L -> the limited signal [L] float32, realigned: the whole hops and the zero-padded tail through one
    StreamLimiter call together with one zero hop that flushes the last one.  kw: StreamLimiter's."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    if x.size == 0:
        raise ValueError("limiter: the input is empty")
    L = x.size
    nh = (L + HOP - 1) // HOP
    d = np.zeros((1, (nh + 1) * HOP), dtype=np.float32)
    d[0, :L] = x
    return StreamLimiter(1, device=device, **kw).process(torch.from_numpy(d))[0, HOP:HOP + L].cpu().numpy()


def build_parser():
    import argparse
    ap = argparse.ArgumentParser(prog='python -m nele_gan_amd.limiter', description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--in', dest='inp', required=True, help='16 kHz PCM_16 wav: what the enhancer or the compressor made, or plain speech')
    ap.add_argument('--out', required=True, help='the limited signal, PCM_16, aligned with the input')
    ap.add_argument('--ceiling-db', type=float, default=-1.0, help='the ceiling, dBFS')
    ap.add_argument('--drive-db', type=float, default=0.0, help='a fixed gain in front of the limiter, dB')
    ap.add_argument('--lookahead-ms', type=float, default=5.0, help='the look-ahead: 1 / 16 ms .. 12 ms')
    ap.add_argument('--release-ms', type=float, default=100.0, help='the release time constant')
    ap.add_argument('--sample-peak', action='store_true', help='detect on the samples only, not between them')
    return ap


def main(argv=None):
    from . import dataio
    ap = build_parser()
    a = ap.parse_args(argv)
    la = int(round(a.lookahead_ms * FS / 1000.0)) if math.isfinite(a.lookahead_ms) else 0
    if not 1 <= la <= MAX_LOOKAHEAD:
        ap.error('--lookahead-ms must give 1 .. %d samples at 16 kHz (%g .. %g ms)' % (MAX_LOOKAHEAD, 1000.0 / FS, 1000.0 * MAX_LOOKAHEAD / FS))
    kw = dict(ceiling_db=a.ceiling_db, drive_db=a.drive_db, lookahead=la, release=a.release_ms / 1000.0, true_peak=not a.sample_peak)
    try:
        release_factor(kw['release'])
        db_factor(a.ceiling_db, '--ceiling-db')
        db_factor(a.drive_db, '--drive-db')
    except ValueError:
        ap.error('--ceiling-db and --drive-db must be finite and --release-ms a time >= 0 whose per-sample factor is below 1')
    wav, sr = dataio.read_wav(a.inp)
    if sr != dataio.fs:
        ap.error('%s is sampled at %d Hz, not %d: convert it first with python -m nele_gan_amd.resample' % (a.inp, sr, dataio.fs))
    if len(wav) == 0:
        ap.error('%s is empty' % a.inp)
    out = limit_file(wav, **kw)
    clipped = int(np.sum(np.abs(out) * np.float32(32767.0) > 32767.5))
    dataio.write_wav_pcm16(a.out, out)
    print('%s: %d samples, limited (ceiling %g dBFS, drive %g dB, look-ahead %d samples, release %g ms, %s peaks): peak %.4f -> %.4f, '
          '%d clipped samples saturated' % (a.out, len(out), a.ceiling_db, a.drive_db, la, a.release_ms, 'sample' if a.sample_peak else 'true',
                                            float(np.abs(wav).max()), float(np.abs(out).max()), clipped))
    return 0


if __name__ == '__main__':
    import sys
    sys.exit(main())
