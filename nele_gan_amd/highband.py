"""The band above 8 kHz past the enhancer: ``HighBandUp`` is the 16 kHz -> device-rate stream converter of the real-time path with the
part of the device-rate input that the 16 kHz path cannot carry added back, delayed to fit (csrc/highband.hip):

    d[n] = enh[n] - g low[n - lam]        u = the stream up-converter's output for d        y[m] = u[m] + g x[m - L]

with low the down-converter's output for x, enh what the enhancer made of it lam = 256 lag_hops samples later and L the delay of x
through down-converter, enhancer and up-converter.  ``RateAdaptedEnhancer(inner, rate, highband=True)`` (nele_gan_amd/streamrate.py)
puts one in the up-converter's place.  This module owns memory and bookkeeping only; there is no arithmetic in torch.

    hb = HighBandUp(streams=256, device_rate=48000)
    y48 = hb.process(enh16, low16, x48)                        # [256, nh * 256] twice, [256, nh * 768] -> [256, nh * 768], hb.lag behind x48

``ScheduledHighBandUp`` is the same on a hop schedule (csrc/highband_sched.hip), for every device rate above
16 kHz, 44.1 kHz and its family among them: the up-converter runs ``shift`` / down of a device sample late, which makes the path's delay
a whole number of samples, ``lag``.  ``FullBandScheduledEnhancer`` and ``adapt_fullband`` (nele_gan_amd/streamrate.py) use it.

    hb = ScheduledHighBandUp(streams=256, device_rate=44100)
    y44 = hb.process(enh16, low16, x44)                        # [256, nh * 256] twice, [256, hb.width_out(nh)] -> the same width, 883 behind x44
"""
import numpy as np
import torch

from . import _lib
from ._lib import c_longlong, call, ptr, stream
from ._slots import HOP, SlotState
from .resample import STREAM_RATE, ScheduledStreamResampler, sched_plan, stream_plan, taps

MAX_LAG16 = _lib.CONSTS7['NELE_HBUP_MAX_LAG16']
MAX_LAG = _lib.CONSTS7['NELE_HBUP_MAX_LAG']


def highband_plan(device_rate, lag_hops=1, quality='high'):
    """The geometry of a HighBandUp -> dict(up, down, zeros, beta, K, hop_out, delay, delay_down, lag16, lag), from the library's host
    functions: no GPU call.  ValueError for a device rate that leaves no band to carry (16 kHz and below), one at which a 16 ms hop is
    not a whole number of samples (44.1 kHz and its family), and one at which the down-converter's delay is not a whole number of
    device-rate samples."""
    device_rate, lag_hops = int(device_rate), int(lag_hops)
    if device_rate <= STREAM_RATE:
        raise ValueError("HighBandUp: a device rate of %d Hz has no band above the %d Hz path's to carry" % (device_rate, STREAM_RATE))
    if (HOP * device_rate) % STREAM_RATE:
        raise ValueError("HighBandUp: at %d Hz a hop is %.4f samples (44.1 kHz and its family): the path's delay is then not a whole "
                         "number of samples - 4414/5 at 44.1 kHz - and an exact complement of the low band needs a fractional delay of "
                         "the input, which is not built (ScheduledHighBandUp and streamrate.adapt_fullband serve these rates: they delay "
                         "the up-converter instead)" % (device_rate, HOP * device_rate / STREAM_RATE))
    if lag_hops < 1:
        raise ValueError("HighBandUp: lag_hops must be >= 1 (got %d)" % lag_hops)
    up, down = stream_plan(STREAM_RATE, device_rate, quality), stream_plan(device_rate, STREAM_RATE, quality)
    n = up['hop_out']
    if (down['delay'] * n) % HOP:
        raise ValueError("HighBandUp: the down-converter's delay of %d samples at %d Hz is %.4f samples at %d Hz, not a whole number: "
                         "the input cannot be delayed to fit" % (down['delay'], STREAM_RATE, down['delay'] * n / HOP, device_rate))
    lag16, lag = HOP * lag_hops, down['delay'] * n // HOP + lag_hops * n + up['delay']
    if lag16 > MAX_LAG16 or lag > MAX_LAG:
        raise ValueError("HighBandUp: lag_hops=%d is a lag of %d samples at %d Hz and %d at %d Hz, above the %d and %d the kernel takes"
                         % (lag_hops, lag16, STREAM_RATE, lag, device_rate, MAX_LAG16, MAX_LAG))
    return {'up': up['up'], 'down': up['down'], 'zeros': up['zeros'], 'beta': up['beta'], 'K': up['K'], 'hop_out': n, 'delay': up['delay'],
            'delay_down': down['delay'], 'lag16': lag16, 'lag': lag}


class HighBandUp(SlotState):
    """``streams`` independent live streams from 16 kHz to ``device_rate`` with the high band of the device-rate input carried.  Per hop
    256 samples of ``enh16`` and ``low16`` and ``hop_out`` samples of ``x_dev`` give ``hop_out`` output samples.  ``delay``: the
    up-converter's own delay D_up; ``lag``: L, how far the output is behind ``x_dev``, = D_down hop_out / 256 + lag_hops hop_out + D_up;
    ``lag_hops``: the hops by which enh16 is behind low16 (1 for a RealtimeEnhancer).  ``gain``: float32 [streams] on the device, g of
    each stream, ones; the caller may overwrite it.  With enh16 = low16 delayed by 256 lag_hops samples the output is x_dev delayed
    by ``lag``, bit for bit.  The state of a slot is its last K - 1 of d, 256 lag_hops of low16 and ``lag`` of x_dev."""

    def __init__(self, streams, device_rate, lag_hops=1, quality='high', device='cuda'):
        super().__init__(streams)
        self.device_rate, self.lag_hops = int(device_rate), int(lag_hops)
        plan = highband_plan(device_rate, lag_hops, quality)   # raises ValueError for an unsupported rate, before any GPU call
        self.up, self.down, self.zeros, self.beta, self.K = plan['up'], plan['down'], plan['zeros'], plan['beta'], plan['K']
        self.hop_out, self.delay, self.lag16, self.lag = plan['hop_out'], plan['delay'], plan['lag16'], plan['lag']
        self._alloc(device, _lib.lib.nele_hbup_state_bytes(self.S, self.K, self.lag16, self.lag))
        self.table = torch.from_numpy(taps(self.up, self.down, self.zeros, self.beta, layout=1)).to(self.device)
        self.gain = torch.ones((self.S,), dtype=torch.float32, device=self.device)
        call('nele_hbup_init', *self._geometry(), stream())

    def _geometry(self):
        return ptr(self.state), c_longlong(self.nbytes), self.S, self.up, self.down, self.K, self.lag16, self.lag

    def _rows(self, t, width, name):
        """a float32 device tensor of ``streams`` rows of ``width`` samples, each contiguous (rows of a wider tensor pass) -> its stride"""
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or tuple(t.shape) != (self.S, width) or t.dtype != torch.float32 or not t.is_cuda \
                or t.stride(1) != 1 or (self.S > 1 and t.stride(0) < width):
            raise ValueError("%s.process: %s must be float32 [%d, %d] on the device with contiguous rows" % (type(self).__name__, name, self.S, width))
        return t.stride(0) if self.S > 1 else width

    def process(self, enh16, low16, x_dev, active=None, out=None):
        """enh16, low16 [streams, nh * 256] at 16 kHz, x_dev [streams, nh * hop_out] at the device rate, float32 on the device (rows of a
        wider tensor pass without a copy: low16 may be rows 0 .. streams - 1 of the down-converter's output) -> y [streams, nh * hop_out]
        on the device, ``lag`` samples behind x_dev.  active: host bool sequence [streams] or None (all): inactive slots are neither
        read nor changed and their output columns are left as they were (give ``out``, a contiguous float32 [streams, nh * hop_out]
        device tensor, to keep them).  Never blocks the host."""
        shape = tuple(np.shape(enh16))
        if len(shape) != 2 or shape[0] != self.S or shape[1] % HOP or shape[1] == 0:
            raise ValueError("HighBandUp.process: enh16 must be [%d, nh * %d] (got %s)" % (self.S, HOP, shape))
        nh = shape[1] // HOP
        se, sl, sx = self._rows(enh16, nh * HOP, 'enh16'), self._rows(low16, nh * HOP, 'low16'), self._rows(x_dev, nh * self.hop_out, 'x_dev')
        act = None if active is None else self._flags(active, "HighBandUp.process: active must hold one flag per stream (%d)" % self.S)
        oshape = (self.S, nh * self.hop_out)
        if out is None:
            out = torch.empty(oshape, dtype=torch.float32, device=self.device)
        elif not isinstance(out, torch.Tensor) or tuple(out.shape) != oshape or out.dtype != torch.float32 or not out.is_cuda \
                or not out.is_contiguous():
            raise ValueError("HighBandUp.process: out must be a contiguous float32 %s tensor on the device" % (oshape,))
        if tuple(self.gain.shape) != (self.S,) or self.gain.dtype != torch.float32 or not self.gain.is_cuda:
            raise ValueError("HighBandUp.process: gain must stay a float32 [%d] tensor on the device" % self.S)
        rows = lambda t: _lib.c_void_p(t.data_ptr())           # checked by _rows: rows of a wider tensor are not contiguous as a whole
        call('nele_hbup_hop', *self._geometry(), ptr(self.table), rows(enh16), c_longlong(se), rows(low16), c_longlong(sl), rows(x_dev),
             c_longlong(sx), ptr(self.gain), ptr(None if act is None else self._dev_bytes(act)), nh, ptr(out), c_longlong(oshape[1]), stream())
        self._count(act, nh)
        return out

    def reset(self, slots):
        """Restart the given slots (zero histories); the other slots, and ``gain``, are not touched."""
        m = self._slots_mask(slots)
        call('nele_hbup_reset', *self._geometry(), ptr(self._dev_bytes(m)), stream())
        self.hops[m] = 0


def highband_sched_plan(device_rate, lag_hops=1, quality='high'):
    """The geometry of a ScheduledHighBandUp -> dict(up, down, zeros, beta, K, delay, delay_down, shift, L0, E, H, lag16, lag, rnum,
    period, hop_min, hop_max), from the library's host functions: no GPU call.  ValueError for a device rate that leaves no band to carry
    (16 kHz and below) and for one the scheduled converters refuse in either direction."""
    device_rate, lag_hops = int(device_rate), int(lag_hops)
    if device_rate <= STREAM_RATE:
        raise ValueError("ScheduledHighBandUp: a device rate of %d Hz has no band above the %d Hz path's to carry" % (device_rate, STREAM_RATE))
    if lag_hops < 1:
        raise ValueError("ScheduledHighBandUp: lag_hops must be >= 1 (got %d)" % lag_hops)
    up, down = sched_plan(STREAM_RATE, device_rate, quality), sched_plan(device_rate, STREAM_RATE, quality)
    info = (_lib.c_int * _lib.CONSTS8['NELE_HBSCHED_INFO'])()
    call('nele_hbsched_plan', up['up'], up['down'], up['zeros'], lag_hops, down['delay'], info)
    at = lambda name: int(info[_lib.CONSTS8['NELE_HBSCHED_I_' + name]])
    return {'up': up['up'], 'down': up['down'], 'zeros': up['zeros'], 'beta': up['beta'], 'K': at('K'), 'delay': at('D_UP'),
            'delay_down': down['delay'], 'shift': at('S'), 'L0': at('L0'), 'E': at('E'), 'H': at('H'), 'lag16': at('LAM'), 'lag': at('LX'),
            'rnum': at('RNUM'), 'period': at('P'), 'hop_min': at('HOP_MIN'), 'hop_max': at('HOP_MAX')}


class ScheduledHighBandUp(SlotState):
    """HighBandUp on ScheduledStreamResampler's hop schedule: ``streams`` independent live streams from 16 kHz to ``device_rate`` with
    the high band of the device-rate input carried, at every rate above 16 kHz the scheduled converters serve.  Per call of nh hops from
    schedule position pos, nh * 256 samples of ``enh16`` and ``low16`` and ``width_out(nh, pos)`` samples of ``x_dev`` give as many
    output samples.  ``delay``: the up-converter's own delay D_up; ``shift``: s, the ticks of 1 / down of a device sample by which the
    up-converter runs late, (-(D_down + 256 lag_hops) up) mod down; ``lag``: Lx, how far the output is behind ``x_dev``, the whole number
    ((D_down + 256 lag_hops) up + s) / down + D_up - 883 at 44.1 kHz where the plain wrapper's latency is 882.8.  ``period``,
    ``positions``, ``position`` and the rules for them are ScheduledStreamResampler's, and so is their code.  ``gain``: float32 [streams]
    on the device, g of each stream, ones; the caller may overwrite it.  With enh16 = low16 delayed by 256 lag_hops samples the output
    is x_dev delayed by ``lag``, bit for bit.  At the whole-hop rates HighBandUp accepts, ``shift`` is 0 and the bits are HighBandUp's."""

    to16k = 0
    _pos, _dev_width, width_in, width_out, call_plan = (ScheduledStreamResampler.__dict__[name] for name in
                                                        ('_pos', '_dev_width', 'width_in', 'width_out', 'call_plan'))

    def __init__(self, streams, device_rate, lag_hops=1, quality='high', device='cuda'):
        super().__init__(streams)
        self.device_rate, self.lag_hops = int(device_rate), int(lag_hops)
        plan = highband_sched_plan(device_rate, lag_hops, quality)   # raises ValueError for an unsupported rate, before any GPU call
        self.up, self.down, self.zeros, self.beta, self.K, self.H = plan['up'], plan['down'], plan['zeros'], plan['beta'], plan['K'], plan['H']
        self.delay, self.shift, self.lag16, self.lag = plan['delay'], plan['shift'], plan['lag16'], plan['lag']
        self.period, self._rnum, self.hop_min, self.hop_max = plan['period'], plan['rnum'], plan['hop_min'], plan['hop_max']
        self.position = 0
        self.positions = np.zeros(self.S, dtype=np.int64)
        self._alloc(device, _lib.lib.nele_hbsched_state_bytes(self.S, self.H, self.lag16, self.lag))
        self.table = torch.from_numpy(taps(self.up, self.down, self.zeros, self.beta, layout=1)).to(self.device)
        self.gain = torch.ones((self.S,), dtype=torch.float32, device=self.device)
        call('nele_hbsched_init', *self._geometry(), stream())

    def _geometry(self):
        return ptr(self.state), c_longlong(self.nbytes), self.S, self.up, self.down, self.K, self.shift, self.lag16, self.lag

    _rows = HighBandUp._rows

    def process(self, enh16, low16, x_dev, active=None, out=None):
        """enh16, low16 [streams, nh * 256] at 16 kHz, x_dev [streams, width_out(nh, pos)] at the device rate, pos the position of the
        active slots, float32 on the device (rows of a wider tensor pass without a copy) -> y of x_dev's shape on the device, ``lag``
        samples behind x_dev.  active: host bool sequence [streams] or None (all): inactive slots are neither read nor changed and their
        output columns are left as they were (give ``out``, a contiguous float32 device tensor of the output's shape, to keep them).
        Never blocks the host."""
        who = type(self).__name__
        shape = tuple(np.shape(enh16))
        if len(shape) != 2 or shape[0] != self.S or shape[1] % HOP or shape[1] == 0:
            raise ValueError("%s.process: enh16 must be [%d, nh * %d] (got %s)" % (who, self.S, HOP, shape))
        act = None if active is None else self._flags(active, "%s.process: active must hold one flag per stream (%d)" % (who, self.S))
        pos, nh = self.call_plan(shape[1], act)                # ValueError: active slots at more than one position
        width = self.width_out(nh, pos)
        se, sl, sx = self._rows(enh16, nh * HOP, 'enh16'), self._rows(low16, nh * HOP, 'low16'), self._rows(x_dev, width, 'x_dev')
        oshape = (self.S, width)
        if out is None:
            out = torch.empty(oshape, dtype=torch.float32, device=self.device)
        elif not isinstance(out, torch.Tensor) or tuple(out.shape) != oshape or out.dtype != torch.float32 or not out.is_cuda \
                or not out.is_contiguous():
            raise ValueError("%s.process: out must be a contiguous float32 %s tensor on the device" % (who, oshape))
        if tuple(self.gain.shape) != (self.S,) or self.gain.dtype != torch.float32 or not self.gain.is_cuda:
            raise ValueError("%s.process: gain must stay a float32 [%d] tensor on the device" % (who, self.S))
        rows = lambda t: _lib.c_void_p(t.data_ptr())           # checked by _rows: rows of a wider tensor are not contiguous as a whole
        call('nele_hbsched_hop', *self._geometry(), ptr(self.table), rows(enh16), c_longlong(se), rows(low16), c_longlong(sl), rows(x_dev),
             c_longlong(sx), ptr(self.gain), ptr(None if act is None else self._dev_bytes(act)), nh, pos, ptr(out), c_longlong(width), stream())
        self._count(act, nh)
        self.positions[slice(None) if act is None else act] = self.position = (pos + nh) % self.period
        return out

    def reset(self, slots, position=None):
        """Restart the given slots (zero histories) at schedule position ``position`` (None: ``position``, where the last process() call
        ended); the other slots, and ``gain``, are not touched."""
        pos = self._pos(position)
        m = self._slots_mask(slots)
        call('nele_hbsched_reset', *self._geometry(), ptr(self._dev_bytes(m)), stream())
        self.hops[m] = 0
        self.positions[m] = pos
