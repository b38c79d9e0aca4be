"""The real-time path at the device's sample rate: ``RateAdaptedEnhancer`` puts a ``StreamResampler`` (nele_gan_amd/resample.py,
csrc/resample_stream.hip) in front of and behind a ``RealtimeEnhancer`` or an ``EchoCancellingEnhancer``, which
work at 16 kHz in hops of 256 samples.  Telephony is 8 kHz, browsers and sound cards 48 kHz; supported device rates are those at which
a 16 ms hop is a whole number of samples (8, 12, 22, 24, 32, 48, 64, 96 kHz ..; not 44.1 kHz and its family - convert those offline with
python -m nele_gan_amd.resample).  ``ScheduledRateEnhancer`` is the same arrangement on ``ScheduledStreamResampler``
(csrc/resample_sched.hip) for every rate, 44.1 kHz and its family among them: the hops at the device rate follow
a schedule (705, 706, 705, 706, 706 samples at 44.1 kHz).  ``adapt`` picks the one that serves a rate.  This module owns memory and
bookkeeping only; there is no arithmetic in torch.

    rt48 = adapt(RealtimeEnhancer(chkpt, streams=256), device_rate=48000)
    out = rt48.process(clean_hops, noise_hops)                 # [256, nh * 768] each, at 48 kHz -> [256, nh * 768] at 48 kHz
    rt44 = adapt(RealtimeEnhancer(chkpt, streams=256), device_rate=44100)
    out = rt44.process(clean_hops, noise_hops)                 # [256, rt44.width(nh)] each, at 44.1 kHz -> the same shape
    full = adapt(RealtimeEnhancer(chkpt, streams=256), device_rate=48000, highband=True)
    out = full.process(clean_hops, noise_hops)                 # the same shapes; what clean_hops holds above 8 kHz is in the output

Without ``highband`` the output is band-limited to the 8 kHz the enhancer works on.  With it a ``HighBandUp`` (nele_gan_amd/highband.py,
csrc/highband.hip) stands in the up-converter's place and adds, in the same launch, the part of ``clean`` that
the 16 kHz path cannot carry, delayed by ``latency``.  ``highband`` is offered where a hop is a whole number of samples;
``adapt_fullband`` gives full-band output at every device rate above 16 kHz, 44.1 kHz and its family among them: there a
``FullBandScheduledEnhancer`` with a ``ScheduledHighBandUp`` (csrc/highband_sched.hip) in the up-converter's place.

    full44 = adapt_fullband(RealtimeEnhancer(chkpt, streams=256), device_rate=44100)
    out = full44.process(clean_hops, noise_hops)               # [256, full44.width(nh)] each -> the same shape, 883 samples behind clean_hops
"""
import fractions

import numpy as np
import torch

from .aec import EchoCancellingEnhancer
from .drc import CompressedEnhancer
from .highband import HighBandUp, ScheduledHighBandUp, highband_plan, highband_sched_plan
from .realtime import HOP, RealtimeEnhancer
from .resample import STREAM_RATE, ScheduledStreamResampler, StreamResampler, stream_plan
from ._slots import dev_f32, dev_rows, host_flags


class RateAdaptedEnhancer:
    """``inner`` (a RealtimeEnhancer or an EchoCancellingEnhancer of B streams) behind one down-converter of 2 B slots - the clean signal
    in slots 0 .. B - 1, the second signal in slots B .. 2 B - 1: one launch, the same delay for both - and in front of an up-converter of
    B slots.  ``hop``: samples per hop at the device rate (device_rate * 16 ms).  ``latency``, in device-rate samples: the down-converter's
    delay (D_down samples at 16 kHz = D_down hop / 256), the enhancer's hop and the up-converter's delay D_up; 960 samples = 20 ms at
    48 kHz with quality 'high'.  device_rate = 16000 passes straight through to ``inner``.

    Around an EchoCancellingEnhancer the two converters' delays are a constant extra delay of the echo path the canceller learns - D_up at
    the device rate plus D_down at 16 kHz, 64 samples at 16 kHz for 48 kHz 'high': leave room for it in the canceller's partitions (DESIGN.md
    section 14).

    ``highband``: None - the output holds the band up to 8 kHz only; True or a float g - a HighBandUp stands in the up-converter's place
    and the output also holds g (1 for True) times what ``clean`` has above that band, time-aligned: one fused launch where the
    up-converter's was.  ``latency`` is then the HighBandUp's ``lag`` for the hops the inner object's output is behind its input: 1 for a
    RealtimeEnhancer, 2 for an EchoCancellingEnhancer whose ``rt`` is a CompressedEnhancer, and the ``lag_hops`` of a
    limiter.LimitedEnhancer there (3 around a CompressedEnhancer; the carried band is added behind the limiter and is not limited).  The canceller never sees the carried band -
    the microphone's down-converter removes it - and a compressor inside the loop acts on the low band only.  ValueError before any GPU
    call at rates that leave no band to carry or at which the path's delay is not a whole number of samples.

    Streams end through drain(): the inner path's finish() and its tails of less than a hop are not offered at the device rate."""

    CONVERTER = StreamResampler
    HIGHBAND = HighBandUp

    def __init__(self, inner, device_rate, quality='high', highband=None):
        if not isinstance(inner, (RealtimeEnhancer, EchoCancellingEnhancer)):
            raise ValueError("%s: inner must be a RealtimeEnhancer or an EchoCancellingEnhancer (got %s)" % (type(self).__name__, type(inner).__name__))
        self.inner, self.S = inner, inner.S
        self.device_rate = int(device_rate)
        self.device = inner.device if isinstance(inner, RealtimeEnhancer) else inner.aec.device
        self._per_call = 1                                 # hops of the last call (an EchoCancellingEnhancer fixes them for its life)
        self.highband = None if highband is None or highband is False else float(highband)     # g; True is 1.0
        if self.device_rate == STREAM_RATE:
            self.down = self.up = self._both = None
            self.hop, self.latency = HOP, HOP
            return
        if self.highband is not None:
            self._check_highband(quality)                  # ValueError before any GPU call
        # both constructors raise ValueError for an unsupported rate before any GPU call
        self.down = self.CONVERTER(2 * self.S, self.device_rate, STREAM_RATE, quality, self.device)
        if self.highband is None:
            self.up = self.CONVERTER(self.S, STREAM_RATE, self.device_rate, quality, self.device)
        else:
            self.up = self.HIGHBAND(self.S, self.device_rate, self._lag_hops(), quality, self.device)
            self.up.gain.fill_(self.highband)
        self._both = None                                  # [2 S, width]: the two signals stacked for the down-converter
        self._set_latency()

    def _lag_hops(self):
        """hops by which the inner object's output is behind its input"""
        rt = self.inner.rt if isinstance(self.inner, EchoCancellingEnhancer) else self.inner
        if hasattr(rt, 'lag_hops'):                        # a limiter.LimitedEnhancer says so itself
            return int(rt.lag_hops)
        return 2 if isinstance(rt, CompressedEnhancer) else 1

    def _check_highband(self, quality):
        if not np.isfinite(self.highband):
            raise ValueError("%s: highband must be None, True or a finite gain (got %r)" % (type(self).__name__, self.highband))
        highband_plan(self.device_rate, self._lag_hops(), quality)

    def _set_latency(self):
        self.hop = self.down.hop_in
        self.latency = self.down.delay * self.hop // HOP + self.hop + self.up.delay if self.highband is None else self.up.lag

    def _stack(self, clean, second, width):
        if self._both is None or self._both.shape[1] != width:
            self._both = torch.empty((2 * self.S, width), dtype=torch.float32, device=self.device)
        shape = (self.S, width)
        who = type(self.down).__name__
        c, s = dev_f32(clean, shape, 'clean', self.device, who), dev_f32(second, shape, 'second', self.device, who)   # both checked before the first copy
        self._both[:self.S].copy_(c, non_blocking=True)
        self._both[self.S:].copy_(s, non_blocking=True)
        return self._both

    def process(self, clean, second, active=None):
        """clean, second [streams, nh * hop] float32 at the device rate (host, pinned host or device); second is the noise for a
        RealtimeEnhancer and the microphone for an EchoCancellingEnhancer -> the enhanced signal [streams, nh * hop] at the device rate,
        on the device, ``latency`` samples behind ``clean``.  active: host bool sequence [streams] or None (all); inactive slots are
        neither read nor changed and their output columns are undefined.  Never blocks the host."""
        if self.down is None:
            self._per_call = max(1, int(np.shape(clean)[-1]) // HOP)
            return self.inner.process(clean, second, active=active)
        shape = tuple(np.shape(clean))
        if len(shape) != 2 or shape[0] != self.S or shape[1] % self.hop or shape[1] == 0:
            raise ValueError("RateAdaptedEnhancer.process: clean must be [%d, nh * %d] (got %s)" % (self.S, self.hop, shape))
        act = None if active is None else host_flags(active, self.S, "RateAdaptedEnhancer.process: active must hold one flag per stream (%d)" % self.S)
        self._per_call = shape[1] // self.hop
        return self._chain(clean, second, shape[1], act)

    def _chain(self, clean, second, width, act):
        low = self.down.process(self._stack(clean, second, width), active=None if act is None else np.concatenate([act, act]))
        out = self.inner.process(low[:self.S], low[self.S:], active=act)
        if self.highband is None:
            return self.up.process(out, active=act)
        return self.up.process(out, low[:self.S], self._both[:self.S], active=act)       # rows of the two buffers: no copy

    def drain(self, slots):
        """ceil(latency / hop) hops of zeros through the given slots -> their outputs [len(slots), ceil(latency / hop) * hop]: what is
        still delayed inside leaves this way (the other slots are not touched).  The zeros go in calls as wide as the last process()
        call (an EchoCancellingEnhancer fixes its hops per call), so those slots may receive a few zero hops more than are returned."""
        slots = np.asarray(slots, dtype=np.int64).reshape(-1)
        act = np.zeros(self.S, dtype=bool)
        act[slots] = True
        nh, per = -(-self.latency // self.hop), self._per_call
        zeros = torch.zeros((self.S, per * self.hop), dtype=torch.float32, device=self.device)
        outs = [self.process(zeros, zeros, active=act) for _ in range(-(-nh // per))]
        rows = dev_rows(slots, self.device)
        return torch.cat([o.index_select(0, rows) for o in outs], dim=1)[:, :nh * self.hop]

    def reset(self, slots):
        """Restart the given slots in the inner object and in both converters."""
        self.inner.reset(slots)
        if self.down is not None:
            slots = np.asarray(slots, dtype=np.int64).reshape(-1)
            self.down.reset(np.concatenate([slots, slots + self.S]))
            self.up.reset(slots)


class ScheduledRateEnhancer(RateAdaptedEnhancer):
    """RateAdaptedEnhancer's arrangement on ScheduledStreamResampler: every device rate section 12 admits, 44.1 kHz and its family among
    them.  Both converters follow the same hop schedule, so a call returns as many samples as it was given: ``width(nh)`` of them for nh
    hops from where the active slots stand (705, 706, 705, 706, 706 per hop at 44.1 kHz).  ``latency`` is a fractions.Fraction in
    device-rate samples, D_down r / 256 + r + D_up with r = 256 device_rate / 16000 samples per hop: 4414 / 5 = 882.8 samples = 20.02 ms
    at 44.1 kHz with quality 'high'.

    Around an EchoCancellingEnhancer the two converters are a constant extra delay of the echo path the canceller learns - D_up at the
    device rate plus D_down at 16 kHz: each stream is the offline conversion of its whole signal, delayed, so nothing in it moves with
    the schedule.

    The slots' schedule positions are the converters' (``down.positions``, ``up.positions``): a call's active slots
    must stand at one position, and reset(slots) starts slots where the last process() call ended."""

    CONVERTER = ScheduledStreamResampler

    def _check_highband(self, quality):
        raise ValueError("ScheduledRateEnhancer: highband is not offered on a hop schedule: the latency there is not a whole number of "
                         "samples (4414/5 at 44.1 kHz), and an exact complement of the low band needs a fractional delay of the input, "
                         "which is not built (FullBandScheduledEnhancer and adapt_fullband carry the band on a hop schedule: they delay "
                         "the up-converter instead)")

    def _set_latency(self):
        r = fractions.Fraction(self.down._rnum, self.down.period)
        self.hop = None                                    # no one hop length: width(nh)
        self.latency = self.down.delay * r / HOP + r + self.up.delay

    def width(self, nh, pos=None):
        """samples per row, at the device rate, of a call of nh hops from schedule position pos (None: where the last call ended)"""
        return nh * HOP if self.down is None else self.down.width_in(nh, pos)

    def process(self, clean, second, active=None):
        """As RateAdaptedEnhancer.process with clean, second [streams, width(nh, pos)], pos the position of the active slots -> the
        enhanced signal of the same shape, ``latency`` samples behind ``clean``."""
        if self.down is None:
            return super().process(clean, second, active=active)
        shape = tuple(np.shape(clean))
        if len(shape) != 2 or shape[0] != self.S or shape[1] == 0:
            raise ValueError("ScheduledRateEnhancer.process: clean must be [%d, width(nh)] (got %s)" % (self.S, shape))
        act = None if active is None else host_flags(active, self.S, "ScheduledRateEnhancer.process: active must hold one flag per stream (%d)" % self.S)
        _, nh = self.down.call_plan(shape[1], None if act is None else np.concatenate([act, act]))      # ValueError: not on the schedule
        self.up.call_plan(nh * HOP, act)
        self._per_call = nh
        return self._chain(clean, second, shape[1], act)

    def drain(self, slots):
        """ceil(latency / r) hops of zeros through the given slots (all at one schedule position) -> their outputs [len(slots), the
        width of those hops from there]: what is still delayed inside leaves this way (the other slots are not touched, and ``position``
        of both converters stays where it was).  The zeros go in calls of as many hops as the last process() call, so those slots may
        receive a few zero hops more than are returned.  reset() them before their next stream."""
        if self.down is None:
            return super().drain(slots)
        slots = np.asarray(slots, dtype=np.int64).reshape(-1)
        act = np.zeros(self.S, dtype=bool)
        act[slots] = True
        r = fractions.Fraction(self.down._rnum, self.down.period)
        nh, per = -(-self.latency // r), self._per_call
        kept = (self.down.position, self.up.position)
        total = self.down.width_in(nh, int(self.down.positions[slots[0]]))
        outs = []
        for _ in range(-(-nh // per)):
            zeros = torch.zeros((self.S, self.down.width_in(per, int(self.down.positions[slots[0]]))), dtype=torch.float32, device=self.device)
            outs.append(self.process(zeros, zeros, active=act))
        self.down.position, self.up.position = kept
        rows = dev_rows(slots, self.device)
        return torch.cat([o.index_select(0, rows) for o in outs], dim=1)[:, :total]

    def reset(self, slots, position=None):
        """Restart the given slots in the inner object and in both converters, at schedule position ``position`` (None: where the last
        process() call ended)."""
        self.inner.reset(slots)
        if self.down is not None:
            slots = np.asarray(slots, dtype=np.int64).reshape(-1)
            self.down.reset(np.concatenate([slots, slots + self.S]), position)
            self.up.reset(slots, position)


class FullBandScheduledEnhancer(ScheduledRateEnhancer):
    """ScheduledRateEnhancer with a ScheduledHighBandUp in the up-converter's place: the output also holds ``gain`` times what ``clean``
    has above the 8 kHz the enhancer works on, time-aligned, at every device rate above 16 kHz - 44.1 kHz and its family among them.  One
    fused launch where the up-converter's was.  ``latency`` is a whole number of device-rate samples, the ScheduledHighBandUp's ``lag``
    for the hops the inner object's output is behind its input (883 at 44.1 kHz with quality 'high' where ScheduledRateEnhancer has
    4414/5: the up-converter runs ``up.shift`` / 160 of a sample late).  16 kHz passes straight through; ValueError before any allocation
    for a rate below 16 kHz, which has no band to carry, and for a gain that is not finite."""

    HIGHBAND = ScheduledHighBandUp

    def __init__(self, inner, device_rate, quality='high', gain=1.0):
        if gain is None or isinstance(gain, bool):
            raise ValueError("FullBandScheduledEnhancer: gain must be a finite number (got %r)" % (gain,))
        super().__init__(inner, device_rate, quality, float(gain))

    def _check_highband(self, quality):
        if not np.isfinite(self.highband):
            raise ValueError("FullBandScheduledEnhancer: gain must be a finite number (got %r)" % self.highband)
        highband_sched_plan(self.device_rate, self._lag_hops(), quality)

    def _set_latency(self):
        self.hop = None                                    # no one hop length: width(nh)
        self.latency = self.up.lag


def adapt_fullband(inner, device_rate, quality='high', gain=1.0):
    """``inner`` at ``device_rate`` with the band above 8 kHz carried, ``gain`` times what ``clean`` holds there: RateAdaptedEnhancer(..,
    highband=gain) where that class accepts the rate, a FullBandScheduledEnhancer otherwise (44.1 kHz and its family; a rate at which
    the path's delay is a fraction of a sample).  16 kHz passes straight through; ValueError for a rate below 16 kHz (no band to carry)."""
    device_rate = int(device_rate)
    if device_rate > STREAM_RATE:
        try:
            highband_plan(device_rate, 1, quality)
        except ValueError:
            return FullBandScheduledEnhancer(inner, device_rate, quality, gain)
    return RateAdaptedEnhancer(inner, device_rate, quality, float(gain))


def adapt(inner, device_rate, quality='high', highband=None):
    """``inner`` at ``device_rate``: a RateAdaptedEnhancer where that class accepts the rate (a 16 ms hop is a whole number of samples;
    16 kHz passes straight through), a ScheduledRateEnhancer otherwise (44.1 kHz and its family).  ``highband``: RateAdaptedEnhancer's;
    a ValueError at the rates of a ScheduledRateEnhancer."""
    device_rate = int(device_rate)
    if device_rate != STREAM_RATE:
        try:
            stream_plan(device_rate, STREAM_RATE, quality)
            stream_plan(STREAM_RATE, device_rate, quality)
        except ValueError:
            return ScheduledRateEnhancer(inner, device_rate, quality, highband)
    return RateAdaptedEnhancer(inner, device_rate, quality, highband)
