"""Real-time, hop-by-hop enhancement of many concurrent streams (near-end listening enhancement at playback time).

``RealtimeEnhancer`` keeps one slot per stream (clean far-end speech + the noise a microphone hears at the listener's end) and turns
every 256-sample hop (16 ms at 16 kHz) of every slot into enhanced speech: the offline chain of ``inference.Enhancer`` run causally -
STFT frame, band features, one IMCRA frame, the causal generator on its running cLN statistics, resynthesis - in libnele_hip.so
(csrc/realtime.hip, the ``nele_rt_*`` entry points).  This module only owns memory and the host-side hop bookkeeping; there is no
arithmetic in torch.  See DESIGN.md "Real-time enhancement" for the contract (alignment, latency, end of stream, normalisation).

    rt = RealtimeEnhancer('chkpt_GD.pt', streams=256)
    out = rt.process(clean_hops, noise_hops)      # [256, nh * 256] in -> [256, nh * 256] out (a slot's first hop: zeros)
    last = rt.finish(slots, clean_tail, noise_tail, tail_lengths)
"""
import numpy as np
import torch

from . import _lib
from . import model as M
from ._lib import c_longlong, call, ptr, stream
from ._slots import SlotState

HOP = 256
NB = 64
_PREC = {'f32': 0, 'bf16': 1}


class RealtimeDebug:
    """Per-frame debug outputs of ``process`` / ``finish``: [streams, frames, 64] float32 each, written at the frame's index (frame t of a
    stream covers its input samples [256 t - 256, 256 t + 256)); frames >= ``frames`` are not written."""

    def __init__(self, streams, frames, device='cuda'):
        z = lambda: torch.zeros((streams, frames, NB), dtype=torch.float32, device=device)
        self.frames = int(frames)
        self.band, self.noise, self.mask, self.alpha2 = z(), z(), z(), z()

    def args(self):
        return [ptr(self.band), ptr(self.noise), ptr(self.mask), ptr(self.alpha2), self.frames]


def _nodbg():
    return [None, None, None, None, 0]


def advance(hops, emitted, live, nh):
    """Host bookkeeping of one process() call (in place): the slots ``live`` receive nh hops; a stream that has received n >= 1 hops has
    emitted 256 (n - 1) samples (output hop h leaves with input hop h + 1)."""
    live = np.asarray(live, dtype=bool)
    emitted[live] += HOP * (np.maximum(hops[live] + nh - 1, 0) - np.maximum(hops[live] - 1, 0))
    hops[live] += nh


class RealtimeEnhancer(SlotState):
    """B independent real-time streams.

    chkpt_path / G: the generator (a checkpoint with an 'enhance-model' entry, or a ``model.Generator_Conv1D_cLN``); random weights when
    neither is given.  precision: 'f32' or 'bf16' (bf16 operands, float32 accumulation, as ``Generator_Conv1D_cLN`` in that mode).
    norm: 'prefix' (alpha^2[t] = mask[t] * sum_{t'<=t} P / sum_{t'<=t} mask P) or a tensor [streams] of fixed beta^2 per slot; the default
    is 'prefix' whatever the checkpoint records.  The matching training and offline modes - the same arithmetic bit for bit - are
    ``train_nele.GanTrainer(norm='prefix')`` and ``inference.Enhancer(norm='prefix')``.

    rule: a ``siiopt.SiiOptRule`` in the generator's place: no checkpoint, no ``G`` and no weights - per hop the
    front kernel and one rule kernel (``nele_rt_rule_hop``); ``precision`` then means nothing.  ``process``, ``finish``, ``reset`` and
    ``RealtimeDebug`` are what they are with a generator, and every wrapper of this class takes the object as it is.

    Host bookkeeping: ``hops[s]`` (hops received), ``emitted[s]`` (output samples produced), ``finished[s]``."""

    def __init__(self, chkpt_path=None, G=None, streams=1, precision='bf16', norm='prefix', device='cuda', rule=None):
        if precision not in _PREC:
            raise ValueError("RealtimeEnhancer: precision must be 'f32' or 'bf16' (got %r)" % (precision,))
        if rule is not None and (chkpt_path is not None or G is not None):
            raise ValueError("RealtimeEnhancer: rule takes the generator's place; pass no chkpt_path and no G with it")
        if rule is not None and not hasattr(rule, 'rt_args'):
            raise ValueError("RealtimeEnhancer: rule must be a siiopt.SiiOptRule")
        super().__init__(streams)
        self._alloc(device, _lib.lib.nele_rt_state_bytes(self.S))
        self.precision = precision
        self.prec = _PREC[precision]
        self.rule = rule
        if G is None and rule is None:
            G = M.Generator_Conv1D_cLN()
            if chkpt_path is not None:
                G.load_state_dict(torch.load(chkpt_path, map_location='cpu')['enhance-model'])
        if isinstance(norm, str):
            if norm != 'prefix':
                raise ValueError("RealtimeEnhancer: norm must be 'prefix' or a tensor of beta^2 per stream")
            self.beta2 = None
        else:
            b2 = torch.as_tensor(norm, dtype=torch.float32).reshape(-1)
            if b2.numel() != self.S:
                raise ValueError("RealtimeEnhancer: norm tensor must hold one beta^2 per stream (%d)" % self.S)
            self.beta2 = b2.to(self.device).contiguous()
        self.emitted = np.zeros(self.S, dtype=np.int64)
        self.finished = np.zeros(self.S, dtype=bool)
        self._params = None
        if rule is not None:
            call('nele_rt_reset', ptr(self.state), c_longlong(self.nbytes), self.S, None, stream())
        else:
            self._load(G, init=True)

    # ---- weights
    def _load(self, G, init):
        G = G.to(self.device)
        flat = G.flat_parameters(self.device).flat
        # a snapshot: later optimiser steps on G must not change the layouts behind this enhancer's back (update_weights does)
        self._params = flat.detach().clone()
        fn = 'nele_rt_init' if init else 'nele_rt_set_weights'
        call(fn, ptr(self.state), c_longlong(self.nbytes), self.S, ptr(self._params), self.prec, stream())

    def update_weights(self, G):
        """Take the current parameters of generator G (e.g. after a training step); the streams' state is kept."""
        if self.rule is not None:
            raise ValueError("RealtimeEnhancer.update_weights: this enhancer runs a rule, it has no weights")
        self._load(G, init=False)

    def _entry(self, what):
        """-> (entry point, the arguments between max_streams and the signals): the generator's precision or the rule's parameters"""
        if self.rule is not None:
            return 'nele_rt_rule_' + what, self.rule.rt_args(self.device)
        return 'nele_rt_' + what, [self.prec]

    # ---- streaming
    def process(self, clean, noise, active=None, debug=None):
        """clean, noise [streams, nh * 256] float32 (host, pinned host or device) -> out [streams, nh * 256] on the device.
        Hop h of a slot (columns 256 h .. 256 h + 255) yields that slot's output hop (m - 1), m = the slot's hop count before it: the
        first hop of a stream yields zeros (16 ms of algorithmic latency).  active: host bool sequence [streams] or None (all); inactive
        slots are neither read nor changed and their output columns are undefined.  Never blocks the host."""
        if clean.dim() != 2 or clean.shape[0] != self.S or clean.shape[1] % HOP or clean.shape[1] == 0:
            raise ValueError("RealtimeEnhancer.process: clean must be [%d, nh * 256]" % self.S)
        nh = clean.shape[1] // HOP
        c = self._dev_f32(clean, (self.S, nh * HOP), 'clean')
        n = self._dev_f32(noise, (self.S, nh * HOP), 'noise')
        act_host = np.ones(self.S, dtype=bool) if active is None \
            else self._flags(active, "RealtimeEnhancer.process: active must hold one flag per stream")
        act = None if active is None else self._dev_bytes(act_host)
        out = torch.empty((self.S, nh * HOP), dtype=torch.float32, device=self.device)
        dbg = debug.args() if debug is not None else _nodbg()
        fn, how = self._entry('hop')
        call(fn, ptr(self.state), c_longlong(self.nbytes), self.S, *how, ptr(c), ptr(n), ptr(act), nh, ptr(self.beta2), ptr(out), *dbg, stream())
        advance(self.hops, self.emitted, act_host & ~self.finished, nh)
        return out

    def finish(self, slots, clean_tail, noise_tail, tail_lengths, debug=None):
        """End the streams of ``slots``: their last r < 256 samples (clean_tail / noise_tail [len(slots), 256], the first
        tail_lengths[i] columns used) -> out [len(slots), 256], the last output hop (from the end-reflected last frame, as the offline
        STFT).  A stream of L samples then has emitted 256 * (L // 256) samples, the offline length.  Streams need >= 2 hops."""
        slots = np.asarray(slots, dtype=np.int64).reshape(-1)
        r = np.asarray(tail_lengths, dtype=np.int64).reshape(-1)
        if r.shape != slots.shape or np.any(r < 0) or np.any(r >= HOP):
            raise ValueError("RealtimeEnhancer.finish: tail_lengths must hold one value in 0 .. 255 per slot")
        if np.any(self.hops[slots] < 2) or np.any(self.finished[slots]):
            raise ValueError("RealtimeEnhancer.finish: every slot needs >= 2 hops and must not be finished")
        ct = torch.as_tensor(clean_tail, dtype=torch.float32).reshape(len(slots), -1)
        nt = torch.as_tensor(noise_tail, dtype=torch.float32).reshape(len(slots), -1)
        if ct.shape[1] != HOP or nt.shape[1] != HOP:
            raise ValueError("RealtimeEnhancer.finish: tails must be [len(slots), 256]")
        idx = torch.from_numpy(slots).to(ct.device)
        full_c = torch.zeros((self.S, HOP), dtype=torch.float32, device=ct.device).index_copy_(0, idx, ct)
        full_n = torch.zeros((self.S, HOP), dtype=torch.float32, device=nt.device).index_copy_(0, idx, nt)
        tails = np.full(self.S, -1, dtype=np.int32)
        tails[slots] = r
        c = self._dev_f32(full_c, (self.S, HOP), 'clean_tail')
        n = self._dev_f32(full_n, (self.S, HOP), 'noise_tail')
        t = torch.from_numpy(tails).pin_memory().to(self.device, non_blocking=True)
        out = torch.empty((self.S, HOP), dtype=torch.float32, device=self.device)
        dbg = debug.args() if debug is not None else _nodbg()
        fn, how = self._entry('finish')
        call(fn, ptr(self.state), c_longlong(self.nbytes), self.S, *how, ptr(c), ptr(n), ptr(t), ptr(self.beta2), ptr(out), *dbg, stream())
        self.emitted[slots] += HOP
        self.finished[slots] = True
        return out.index_select(0, torch.from_numpy(slots).to(self.device))

    def reset(self, slots):
        """Restart the given slots (a fresh IMCRA estimator, zeroed histories and cLN sums); the other slots are not touched."""
        m = self._slots_mask(slots)
        call('nele_rt_reset', ptr(self.state), c_longlong(self.nbytes), self.S, ptr(self._dev_bytes(m)), stream())
        self.hops[m] = 0
        self.emitted[m] = 0
        self.finished[m] = False
