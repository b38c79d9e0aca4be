"""Audio at any sample rate to the rate the package works at: a rational-ratio polyphase FIR resampler on the GPU (csrc/resample.hip; the
operation is fixed by DESIGN.md section 12 - scipy.signal.resample_poly's convention with a Kaiser-windowed sinc).  The reference loads
files at their own rate and asserts 16 kHz (dataloader.py:34-37): this is an addition to it, not a parity item.

    Resampler(sr_in, sr_out=16000, quality='high').apply(wav, lengths) -> (y, lengths_out)        device tensors [B, L]
    resample(wav, lengths, sr_in, sr_out=16000, quality='high')        -> (y, lengths_out)        sr_in: an int, or one per row
    python -m nele_gan_amd.resample --in DIR --out DIR [--sr 16000] [--quality high|scipy] [--batch 64]
                                                                       every .wav under DIR as PCM_16 at --sr, same relative path,
                                                                       and DIR/resample_manifest.csv
    StreamResampler(streams, sr_in, sr_out, quality='high').process(x_hops) -> y_hops             live streams hop by hop between 16 kHz and
                                                                       8 .. 96 kHz (csrc/resample_stream.hip)
    ScheduledStreamResampler(streams, sr_in, sr_out, quality='high').process(x) -> y              the same for every rate, 44.1 kHz and its
                                                                       family among them, on a hop schedule (csrc/resample_sched.hip,
                                                                       DESIGN.md section 20)

``quality``: 'high' = (zeros 32, Kaiser beta 12.0): stop band at most -119 dB from 1.15 x the new Nyquist frequency, pass-band ripple below
0.001 dB up to 0.85 x; 'scipy' = (10, 5.0): resample_poly's own default (-43 dB); or a (zeros, beta) pair.  The taps are designed on the
host by the library (nele_resample_taps: no GPU needed).  A row's output bits do not depend on the batch it is in.
"""
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import c_int, c_longlong, c_void_p, call, ptr, stream
from ._slots import SlotState

QUALITIES = {'high': (32, 12.0), 'scipy': (10, 5.0)}
MAX_SAMPLES = _lib.CONSTS['NELE_RESAMPLE_MAX_SAMPLES']
MANIFEST_COLUMNS = ('name', 'sr_in', 'samples_in', 'samples_out', 'peak', 'clipped_samples')

TILE = int(_lib.lib.nele_resample_tile())                  # outputs per workgroup of the kernel (tests put lengths around it)

# the stream converter of the real-time path (csrc/resample_stream.hip)
STREAM_RATE = 16000                                        # the rate of the real-time path: one side of every stream converter


def ratio(sr_in, sr_out):
    """-> (up, down) = sr_out / sr_in in lowest terms"""
    sr_in, sr_out = int(sr_in), int(sr_out)
    if sr_in < 1 or sr_out < 1:
        raise ValueError("resample: sample rates must be positive (got %d -> %d)" % (sr_in, sr_out))
    g = math.gcd(sr_in, sr_out)
    return sr_out // g, sr_in // g


def quality_params(quality):
    """'high' | 'scipy' | (zeros, beta) -> (zeros, beta)"""
    if isinstance(quality, str):
        if quality not in QUALITIES:
            raise ValueError("resample: quality must be one of %s or a (zeros, beta) pair" % sorted(QUALITIES))
        return QUALITIES[quality]
    zeros, beta = quality
    return int(zeros), float(beta)


def out_len(n_in, up, down):
    """ceil(n_in up / down): scipy.signal.resample_poly's output length (nele_resample_out_len)"""
    n = int(_lib.lib.nele_resample_out_len(int(n_in), int(up), int(down)))
    if n < 0:
        _lib.check(-1, 'nele_resample_out_len')
    return n


def taps_count(up, down, zeros, layout):
    """2 half + 1 taps (layout 0) or the up * K entries of the polyphase table (layout 1), as the library counts them"""
    n = int(_lib.lib.nele_resample_taps_count(int(up), int(down), int(zeros), int(layout)))
    if n < 0:
        _lib.check(-1, 'nele_resample_taps_count')
    return n


def taps(up, down, zeros=32, beta=12.0, layout=0):
    """The filter as the library designs it on the host (nele_resample_taps), float64: layout 0 the taps h[0 .. 2 half] in natural order,
    layout 1 the polyphase table hp[up][K]."""
    out = np.empty(taps_count(up, down, zeros, layout), dtype=np.float64)
    call('nele_resample_taps', int(up), int(down), int(zeros), float(beta), int(layout), c_void_p(out.ctypes.data))
    return out.reshape(int(up), -1) if layout == 1 else out


def _host_lengths(lengths, B):
    if isinstance(lengths, torch.Tensor):
        lengths = lengths.detach().cpu().numpy()
    h = np.ascontiguousarray(np.asarray(lengths).reshape(-1), dtype=np.int64)
    if h.shape != (B,):
        raise ValueError("resample: lengths must hold one entry per row (%d), got %d" % (B, h.size))
    return h


class Resampler:
    """One rate pair and one filter: the table is designed and uploaded once."""

    def __init__(self, sr_in, sr_out=16000, quality='high', device='cuda'):
        self.sr_in, self.sr_out = int(sr_in), int(sr_out)
        self.up, self.down = ratio(sr_in, sr_out)
        self.zeros, self.beta = quality_params(quality)
        table = taps(self.up, self.down, self.zeros, self.beta, layout=1)          # raises ValueError outside the supported ratios
        self.K = int(table.shape[1])
        self.device = torch.device(device)
        self.table = torch.from_numpy(table).to(self.device)

    def out_len(self, n):
        return out_len(n, self.up, self.down)

    def apply(self, wav, lengths, row_ids=None, out=None, gain=1.0):
        """wav float32 [B, Lmax] on the device, lengths [B] (host or device) -> (y float32 [B, Lmax_out], lengths_out int32 [B]) with exact
        zeros behind each row's output length.  row_ids: the rows to process (others are neither read nor written; None: all).
        out: a (y, lengths_out) pair to write into - y [B, >= the longest output] float32, lengths_out [B] int32, both on the device."""
        if wav.dim() != 2 or wav.dtype != torch.float32 or wav.shape[0] == 0 or wav.shape[1] == 0:
            raise ValueError("resample: wav must be a float32 [B, Lmax] tensor, not empty")
        x = ptr(wav)                                         # raises on a host tensor: there is no CPU path
        B, L = wav.shape
        host = _host_lengths(lengths, B)
        if (host < 0).any() or (host > L).any():
            raise ValueError("resample: lengths must lie in 0 .. %d" % L)
        if L > MAX_SAMPLES:
            raise ValueError("resample: rows of more than 2^30 samples are not supported")
        rows = np.arange(B) if row_ids is None else np.asarray(row_ids.cpu() if isinstance(row_ids, torch.Tensor) else row_ids, dtype=np.int64).reshape(-1)
        if rows.size == 0 or (rows < 0).any() or (rows >= B).any():
            raise ValueError("resample: row_ids must name rows 0 .. %d" % (B - 1))
        need = max(1, max(self.out_len(int(host[r])) for r in rows))
        dev = wav.device
        if out is None:
            y = torch.empty((B, need), dtype=torch.float32, device=dev) if row_ids is None else torch.zeros((B, need), dtype=torch.float32, device=dev)
            n_out = torch.zeros((B,), dtype=torch.int32, device=dev)
        else:
            y, n_out = out
            if y.dim() != 2 or y.dtype != torch.float32 or y.shape[0] != B or y.shape[1] < need or y.device != dev:
                raise ValueError("resample: out[0] must be float32 [%d, >= %d] on %s" % (B, need, dev))
            if n_out.dtype != torch.int32 or n_out.shape != (B,) or n_out.device != dev:
                raise ValueError("resample: out[1] must be int32 [%d] on %s" % (B, dev))
        ln = lengths if (isinstance(lengths, torch.Tensor) and lengths.dtype == torch.int32 and lengths.device == dev and lengths.is_contiguous()) \
            else torch.from_numpy(host.astype(np.int32)).to(dev)
        ids = None if row_ids is None else torch.from_numpy(rows.astype(np.int32)).to(dev)
        table = self.table if self.table.device == dev else self.table.to(dev)
        call('nele_resample_var', x, L, ptr(ln), ptr(ids), int(rows.size), int(y.shape[1]), self.up, self.down, self.K, ptr(table), float(gain),
             ptr(y), int(y.shape[1]), ptr(n_out), stream())
        return y, n_out


def stream_plan(sr_in, sr_out, quality='high'):
    """The stream converter sr_in -> sr_out of DESIGN.md section 15 -> dict(up, down, zeros, beta, K, hop_in, hop_out, delay), from the
    library's host functions: no GPU call.  One side must be 16 000 Hz and a 256-sample hop there a whole number of samples on the
    other side; anything else is a ValueError (44.1 kHz and its family: convert those offline, python -m nele_gan_amd.resample)."""
    sr_in, sr_out = int(sr_in), int(sr_out)
    up, down = ratio(sr_in, sr_out)
    if STREAM_RATE not in (sr_in, sr_out):
        raise ValueError("StreamResampler: one side must be %d Hz, the rate of the real-time path (got %d -> %d); other pairs are converted "
                         "offline, by Resampler / python -m nele_gan_amd.resample" % (STREAM_RATE, sr_in, sr_out))
    zeros, beta = quality_params(quality)
    n_in, n_out = c_int(0), c_int(0)
    call('nele_resample_stream_hop_lengths', up, down, int(sr_out == STREAM_RATE), ctypes.byref(n_in), ctypes.byref(n_out))
    delay = int(_lib.lib.nele_resample_stream_delay(up, down, zeros))
    if delay < 0:
        _lib.check(-1, 'nele_resample_stream_delay')
    if delay > n_out.value:
        raise ValueError("StreamResampler: the filter's delay of %d output samples is longer than a hop of %d" % (delay, n_out.value))
    K = taps_count(up, down, zeros, 1) // up                # the table is hp[up][K]
    return {'up': up, 'down': down, 'zeros': zeros, 'beta': beta, 'K': K, 'hop_in': n_in.value, 'hop_out': n_out.value, 'delay': delay}


class StreamResampler(SlotState):
    """``streams`` independent live streams from sr_in to sr_out, hop by hop (csrc/resample_stream.hip; the arithmetic is DESIGN.md
    section 15).  One side is 16 kHz, where a hop is 256 samples: ``hop_in`` input samples give ``hop_out`` output samples.  What a stream
    has emitted is, bit for bit, ``Resampler(sr_in, sr_out, quality)``'s output for the whole signal fed so far, ``delay`` output samples
    late (the first ``delay`` outputs are the filter's pre-ringing); flush() hands out the rest.  The state of a slot is its last K - 1
    input samples.  This class owns memory and bookkeeping only; there is no arithmetic in torch."""

    def __init__(self, streams, sr_in, sr_out, quality='high', device='cuda'):
        super().__init__(streams)
        self.sr_in, self.sr_out = int(sr_in), int(sr_out)
        plan = stream_plan(sr_in, sr_out, quality)           # raises ValueError for an unsupported pair, before any GPU call
        self.up, self.down, self.zeros, self.beta, self.K = plan['up'], plan['down'], plan['zeros'], plan['beta'], plan['K']
        self.hop_in, self.hop_out, self.delay = plan['hop_in'], plan['hop_out'], plan['delay']
        self._alloc(device, _lib.lib.nele_resample_stream_state_bytes(self.S, self.K))
        self.table = torch.from_numpy(taps(self.up, self.down, self.zeros, self.beta, layout=1)).to(self.device)
        self._zero_hop = None
        call('nele_resample_stream_init', ptr(self.state), c_longlong(self.nbytes), self.S, self.up, self.down, self.K, stream())

    # ---- streaming
    def process(self, x, active=None, out=None):
        """x [streams, nh * hop_in] float32 (host, pinned host or device) -> y [streams, nh * hop_out] on the device.  active: host bool
        sequence [streams] or None (all): inactive slots are neither read nor changed and their output columns are left as they were
        (undefined in a fresh tensor; give ``out``, a float32 [streams, nh * hop_out] device tensor, to keep them).  Never blocks the
        host."""
        shape = tuple(np.shape(x))
        if len(shape) != 2 or shape[0] != self.S or shape[1] % self.hop_in or shape[1] == 0:
            raise ValueError("StreamResampler.process: x must be [%d, nh * %d] (got %s)" % (self.S, self.hop_in, shape))
        nh = shape[1] // self.hop_in
        act = None if active is None else self._flags(active, "StreamResampler.process: active must hold one flag per stream (%d)" % self.S)
        oshape = (self.S, nh * self.hop_out)
        if out is None:
            out = torch.empty(oshape, dtype=torch.float32, device=self.device)
        elif not isinstance(out, torch.Tensor) or tuple(out.shape) != oshape or out.dtype != torch.float32 or not out.is_cuda \
                or not out.is_contiguous():
            raise ValueError("StreamResampler.process: out must be a contiguous float32 %s tensor on the device" % (oshape,))
        xd = self._dev_f32(x, shape, 'x')                     # every check is behind us: the first transfer
        call('nele_resample_stream_hop', ptr(self.state), c_longlong(self.nbytes), self.S, self.up, self.down, self.K, ptr(self.table), ptr(xd),
             c_longlong(shape[1]), ptr(None if act is None else self._dev_bytes(act)), nh, self.hop_in, ptr(out), c_longlong(oshape[1]), stream())
        self.hops[slice(None) if act is None else act] += nh
        return out

    def flush(self, slots):
        """End the streams of ``slots``: one hop of zeros through those slots -> its first ``delay`` columns, [len(slots), delay] - the
        outputs still inside the filter; with what was emitted that is the offline resampler's whole output.  Resets those slots."""
        slots = np.asarray(slots, dtype=np.int64).reshape(-1)
        if self._zero_hop is None:
            self._zero_hop = torch.zeros((self.S, self.hop_in), dtype=torch.float32, device=self.device)
        y = self.process(self._zero_hop, active=self._slots_mask(slots))
        tail = y.index_select(0, self._dev_rows(slots))[:, :self.delay].contiguous()
        self.reset(slots)
        return tail

    def reset(self, slots):
        """Restart the given slots (a zero history); the other slots are not touched."""
        m = self._slots_mask(slots)
        call('nele_resample_stream_reset', ptr(self.state), c_longlong(self.nbytes), self.S, self.up, self.down, self.K, ptr(self._dev_bytes(m)),
             stream())
        self.hops[m] = 0


def sched_plan(sr_in, sr_out, quality='high'):
    """The scheduled stream converter sr_in -> sr_out of DESIGN.md section 20 -> dict(up, down, zeros, beta, to16k, K, delay, L0, E, H,
    rnum, period, hop_min, hop_max), from the library's host function nele_sched_stream_plan: no GPU call.  One side must be 16 000 Hz;
    r = rnum / period device-side samples per hop."""
    sr_in, sr_out = int(sr_in), int(sr_out)
    up, down = ratio(sr_in, sr_out)
    if STREAM_RATE not in (sr_in, sr_out):
        raise ValueError("ScheduledStreamResampler: one side must be %d Hz, the rate of the real-time path (got %d -> %d); other pairs are "
                         "converted offline, by Resampler / python -m nele_gan_amd.resample" % (STREAM_RATE, sr_in, sr_out))
    zeros, beta = quality_params(quality)
    to16k = int(sr_out == STREAM_RATE)
    info = (c_int * _lib.CONSTS3['NELE_SCHED_INFO'])()
    call('nele_sched_stream_plan', up, down, zeros, to16k, info)
    at = lambda name: int(info[_lib.CONSTS3['NELE_SCHED_I_' + name]])
    return {'up': up, 'down': down, 'zeros': zeros, 'beta': beta, 'to16k': to16k, 'K': at('K'), 'delay': at('D'), 'L0': at('L0'), 'E': at('E'),
            'H': at('H'), 'rnum': at('RNUM'), 'period': at('P'), 'hop_min': at('HOP_MIN'), 'hop_max': at('HOP_MAX')}


class ScheduledStreamResampler(SlotState):
    """``streams`` independent live streams from sr_in to sr_out on a hop schedule (csrc/resample_sched.hip; the arithmetic is DESIGN.md
    section 20): StreamResampler for every rate, 44.1 kHz and its family among them.  One side is 16 kHz, where a hop is 256 samples; on
    the other side the hop at schedule position g has floor((g + 1) r) - floor(g r) samples, r = 256 sr_dev / 16000 (705, 706, 705, 706,
    706 at 44.1 kHz), repeating with ``period``.  What a stream has emitted is, bit for bit, ``Resampler(sr_in, sr_out, quality)``'s
    output for the whole signal fed so far, ``delay`` output samples late; flush() hands out the rest.

    The schedule positions live here, on the host: ``positions[slot]``, and ``position``, where the last process() call ended - where
    reset() starts a slot, so that a fresh stream joins the running ones in step.  A call runs its hops from one position: all its
    active slots must stand there.  A slot that sat out k hops is in step again when k is a multiple of ``period``; until then it runs
    in calls of its own or is reset.  This class owns memory and bookkeeping only; there is no arithmetic in torch."""

    def __init__(self, streams, sr_in, sr_out, quality='high', device='cuda'):
        super().__init__(streams)
        self.sr_in, self.sr_out = int(sr_in), int(sr_out)
        plan = sched_plan(sr_in, sr_out, quality)            # raises ValueError for an unsupported pair, before any GPU call
        self.up, self.down, self.zeros, self.beta, self.to16k = plan['up'], plan['down'], plan['zeros'], plan['beta'], plan['to16k']
        self.K, self.H, self.delay, self.period, self._rnum = plan['K'], plan['H'], plan['delay'], plan['period'], plan['rnum']
        self.hop_min, self.hop_max = plan['hop_min'], plan['hop_max']
        self.position = 0
        self.positions = np.zeros(self.S, dtype=np.int64)
        self._alloc(device, _lib.lib.nele_sched_stream_state_bytes(self.S, self.H))
        self.table = torch.from_numpy(taps(self.up, self.down, self.zeros, self.beta, layout=1)).to(self.device)
        call('nele_sched_stream_init', *self._geometry(), stream())

    def _geometry(self):
        return ptr(self.state), c_longlong(self.nbytes), self.S, self.up, self.down, self.K, self.to16k

    # ---- the schedule
    def _pos(self, pos):
        pos = self.position if pos is None else int(pos)
        if not 0 <= pos < self.period:
            raise ValueError("%s: position %d outside 0 .. %d" % (type(self).__name__, pos, self.period - 1))
        return pos

    def _dev_width(self, nh, pos):
        return (pos + nh) * self._rnum // self.period - pos * self._rnum // self.period

    def width_in(self, nh, pos=None):
        """input samples per row of a call of nh hops from schedule position pos (None: ``position``)"""
        return self._dev_width(int(nh), self._pos(pos)) if self.to16k else int(nh) * TILE

    def width_out(self, nh, pos=None):
        """output samples per row of a call of nh hops from schedule position pos (None: ``position``)"""
        return int(nh) * TILE if self.to16k else self._dev_width(int(nh), self._pos(pos))

    def call_plan(self, width, act=None):
        """(pos, nh) of a call whose rows are ``width`` input samples wide in the slots of the host mask ``act`` (None: all): the
        position those slots stand at and the hops the width is from there.  ValueError names the slots that stand elsewhere, or says
        that the width is not one of the schedule's."""
        who = type(self).__name__
        at = self.positions if act is None else self.positions[act]
        pos = self.position if at.size == 0 else int(np.bincount(at).argmax())
        if (at != pos).any():
            idx = np.arange(self.S) if act is None else np.nonzero(act)[0]
            raise ValueError("%s.process: slots %s stand at schedule positions %s, the call's other slots at %d: run them in calls of their own "
                             "or reset them" % (who, idx[at != pos].tolist(), at[at != pos].tolist(), pos))
        width = int(width)
        nh = width * self.period // self._rnum if self.to16k else width // TILE      # widths grow strictly with nh: this or the next
        for n in (nh, nh + 1):
            if n >= 1 and self.width_in(n, pos) == width:
                return pos, n
        raise ValueError("%s.process: x must be [%d, width] with a width of the schedule from position %d - %d, %d, %d, .. (got %d)"
                         % (who, self.S, pos, self.width_in(1, pos), self.width_in(2, pos), self.width_in(3, pos), width))

    # ---- streaming
    def process(self, x, active=None, out=None):
        """x [streams, width_in(nh, pos)] float32 (host, pinned host or device), pos the position of the active slots -> y [streams,
        width_out(nh, pos)] on the device.  active: host bool sequence [streams] or None (all): inactive slots are neither read nor
        changed and their output columns are left as they were (undefined in a fresh tensor; give ``out``, a float32 device tensor of
        the output's shape, to keep them).  Never blocks the host."""
        who = type(self).__name__
        shape = tuple(np.shape(x))
        if len(shape) != 2 or shape[0] != self.S or shape[1] == 0:
            raise ValueError("%s.process: x must be [%d, width] (got %s)" % (who, self.S, shape))
        if isinstance(x, torch.Tensor) and x.dtype != torch.float32:
            raise ValueError("%s: x must be float32" % who)
        act = None if active is None else self._flags(active, "%s.process: active must hold one flag per stream (%d)" % (who, self.S))
        pos, nh = self.call_plan(shape[1], act)
        oshape = (self.S, self.width_out(nh, pos))
        if out is None:
            out = torch.empty(oshape, dtype=torch.float32, device=self.device)
        elif not isinstance(out, torch.Tensor) or tuple(out.shape) != oshape or out.dtype != torch.float32 or not out.is_cuda \
                or not out.is_contiguous():
            raise ValueError("%s.process: out must be a contiguous float32 %s tensor on the device" % (who, oshape))
        xd = self._dev_f32(x, shape, 'x')                     # every check is behind us: the first transfer
        call('nele_sched_stream_hop', *self._geometry(), ptr(self.table), ptr(xd), c_longlong(shape[1]),
             ptr(None if act is None else self._dev_bytes(act)), nh, pos, ptr(out), c_longlong(oshape[1]), stream())
        which = slice(None) if act is None else act
        self.hops[which] += nh
        self.positions[which] = self.position = (pos + nh) % self.period
        return out

    def flush(self, slots):
        """End the streams of ``slots`` (all at one position): one hop of zeros through those slots -> its first ``delay`` columns,
        [len(slots), delay] - the outputs still inside the filter; with what was emitted that is the offline resampler's whole output.
        Resets those slots to ``position``, which this call leaves where it was."""
        slots = np.asarray(slots, dtype=np.int64).reshape(-1)
        mask, position = self._slots_mask(slots), self.position
        pos = int(self.positions[slots[0]]) if slots.size else position
        y = self.process(torch.zeros((self.S, self.width_in(1, pos)), dtype=torch.float32, device=self.device), active=mask)
        tail = y.index_select(0, self._dev_rows(slots))[:, :self.delay].contiguous()
        self.position = position
        self.reset(slots)
        return tail

    def reset(self, slots, position=None):
        """Restart the given slots (a zero history) at schedule position ``position`` (None: ``position``, where the last process()
        call ended); the other slots are not touched."""
        pos = self._pos(position)
        m = self._slots_mask(slots)
        call('nele_sched_stream_reset', *self._geometry(), ptr(self._dev_bytes(m)), stream())
        self.hops[m] = 0
        self.positions[m] = pos


_CACHE = {}


def resampler(sr_in, sr_out=16000, quality='high', device='cuda'):
    """The Resampler of (sr_in, sr_out, quality, device), built once per process."""
    key = (int(sr_in), int(sr_out), quality if isinstance(quality, str) else tuple(quality), str(torch.device(device)))
    r = _CACHE.get(key)
    if r is None:
        r = _CACHE[key] = Resampler(sr_in, sr_out, quality, device)
    return r


def resample(wav, lengths, sr_in, sr_out=16000, quality='high', gain=1.0):
    """wav float32 [B, Lmax] on the device, lengths [B]; sr_in an int or one int per row -> (y [B, max n_out], lengths_out int32 [B]).
    Rows with different rates are grouped: one kernel call per distinct rate on the rows it names; rows already at sr_out are copied."""
    if not isinstance(wav, torch.Tensor) or not wav.is_cuda:
        raise ValueError("nele_gan_amd: expected a tensor on the GPU (got %s)" % (wav.device if isinstance(wav, torch.Tensor) else type(wav).__name__))
    if np.ndim(sr_in) == 0:
        return resampler(int(sr_in), sr_out, quality, wav.device).apply(wav, lengths, gain=gain)
    B = wav.shape[0]
    rates = np.asarray(sr_in, dtype=np.int64).reshape(-1)
    if rates.shape != (B,):
        raise ValueError("resample: sr_in must be an int or hold one rate per row (%d)" % B)
    host = _host_lengths(lengths, B)
    groups = {int(r): np.nonzero(rates == r)[0] for r in sorted(set(rates.tolist()))}
    res = {r: resampler(r, sr_out, quality, wav.device) for r in groups}
    need = max(1, max(res[int(r)].out_len(int(n)) for r, n in zip(rates, host)))
    y = torch.empty((B, need), dtype=torch.float32, device=wav.device)           # every row is named by one of the calls
    n_out = torch.empty((B,), dtype=torch.int32, device=wav.device)
    ln = torch.from_numpy(host.astype(np.int32)).to(wav.device)
    for r, rows in groups.items():
        res[r].apply(wav, ln, row_ids=rows, out=(y, n_out), gain=gain)
    return y, n_out


def resample_host(x, sr_in, sr_out=16000, quality='high', gain=1.0, device='cuda'):
    """One host signal (1-D float32 array) through the device resampler -> float32 array of out_len samples."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1))
    if len(x) == 0 or int(sr_in) == int(sr_out) and gain == 1.0:
        return x
    y, n = resampler(sr_in, sr_out, quality, device).apply(torch.from_numpy(x).to(device).unsqueeze(0), [len(x)], gain=gain)
    return y[0, :int(n[0])].cpu().numpy()


# ------------------------------------------------------------------------------------------------ a folder of files at any rate
def _convert_batch(items, sr_in, sr_out, quality, out_dir, device, workers):
    """items: [(relative name, float32 signal)] at sr_in -> PCM_16 files under out_dir and their manifest rows.  Samples PCM_16 cannot
    hold are saturated in the file and counted."""
    from . import dataio
    from .ssdrc import pcm16_codes
    lens = np.asarray([len(x) for _, x in items], dtype=np.int32)
    rows = np.zeros((len(items), max(1, int(lens.max()))), dtype=np.float32)
    for k, (_, x) in enumerate(items):
        rows[k, :len(x)] = x
    y, n_out = resample(torch.from_numpy(rows).to(device), lens, int(sr_in), sr_out, quality)
    codes = pcm16_codes(y)
    clipped = (torch.abs(y) * 32767.0 > 32767.5).sum(dim=1).cpu().numpy()
    peak = torch.abs(y).amax(dim=1).cpu().numpy()
    n_host = n_out.cpu().numpy().astype(np.int32)
    paths = [os.path.join(out_dir, nm) for nm, _ in items]
    for p in paths:
        dataio.creatdir(os.path.dirname(p))
    dataio.write_wav_batch_pcm16(paths, np.ascontiguousarray(codes.to(torch.int16).cpu().numpy()), n_host, sr=int(sr_out), threads=workers)
    return [(nm, int(sr_in), int(lens[k]), int(n_host[k]), '%.9g' % float(peak[k]), int(clipped[k])) for k, (nm, _) in enumerate(items)]


def write_manifest(out_dir, rows):
    import csv
    with open(os.path.join(out_dir, 'resample_manifest.csv'), 'w', newline='') as fh:
        w = csv.writer(fh, lineterminator='\n')
        w.writerow(MANIFEST_COLUMNS)
        w.writerows(rows)


def resample_corpus(in_dir, out_dir, sr=16000, quality='high', batch=64, workers=8, device='cuda'):
    """Every .wav under in_dir (any RIFF flavour dataio.read_wav reads, mixed to mono) as PCM_16 at ``sr`` under the same relative path
    in out_dir, and out_dir/resample_manifest.csv -> manifest rows (sorted by name).  Files are batched by their rate; files already at
    ``sr`` are rewritten as PCM_16 without filtering."""
    from . import dataio
    files = sorted(dataio.get_filepaths(in_dir))
    dataio.creatdir(out_dir)
    pending, rows = {}, []
    for f in files:
        x, file_sr = dataio.read_wav(f)
        group = pending.setdefault(int(file_sr), [])
        group.append((os.path.relpath(f, in_dir), x))
        if len(group) >= batch:
            rows += _convert_batch(group, file_sr, sr, quality, out_dir, device, workers)
            pending[int(file_sr)] = []
    for file_sr, group in sorted(pending.items()):
        if group:
            rows += _convert_batch(group, file_sr, sr, quality, out_dir, device, workers)
    rows.sort(key=lambda r: r[0])
    write_manifest(out_dir, rows)
    return rows


def main(argv=None):
    import argparse
    from . import dataio
    ap = argparse.ArgumentParser(prog='python -m nele_gan_amd.resample', description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--in', dest='src', required=True, help='folder of wav files at any sample rate')
    ap.add_argument('--out', required=True, help='folder the converted files and resample_manifest.csv are written under')
    ap.add_argument('--sr', type=int, default=16000, help='the rate to convert to')
    ap.add_argument('--quality', choices=sorted(QUALITIES), default='high')
    ap.add_argument('--batch', type=int, default=64, help='files of one rate per kernel call')
    a = ap.parse_args(argv)
    if a.batch < 1 or a.sr < 1:
        ap.error('--batch and --sr must be positive')
    if not dataio.get_filepaths(a.src):
        ap.error('no wav file under %s' % a.src)
    rows = resample_corpus(a.src, a.out, sr=a.sr, quality=a.quality, batch=a.batch)
    print('%d files at %d Hz under %s (%d resampled, %d with clipped samples - see resample_manifest.csv)'
          % (len(rows), a.sr, a.out.rstrip('/'), sum(1 for r in rows if r[1] != a.sr), sum(1 for r in rows if r[5] != 0)))
    return 0


if __name__ == '__main__':
    import sys
    sys.exit(main())
