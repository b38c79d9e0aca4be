"""Host side of the per-stream slot state (csrc/slot_state.h): what ``RealtimeEnhancer``, ``EchoCanceller`` and ``StreamResampler`` share -
the slot count, the device, the hop counters, and the ways their arguments reach the device without blocking the host.  Messages carry
the name of the class that raises them."""
import numpy as np
import torch

from ._lib import norm_dev

HOP = 256                                                  # samples per hop of every hop-wise slot class


def to_dev(t, device):
    """host tensor -> device through pinned memory, without blocking the host"""
    if t.device == device or device.type != 'cuda':
        return t.to(device)
    return (t if t.is_pinned() else t.pin_memory()).to(device, non_blocking=True)


def host_flags(flags, S, text):
    """host bool sequence [S] -> bool array; ``text``: the message when it does not hold one flag per stream"""
    m = np.asarray(flags, dtype=bool).reshape(-1)
    if m.shape[0] != S:
        raise ValueError(text)
    return m


def dev_rows(slots, device):
    """slot list -> int64 row indices on the device (for index_select / index_copy_)"""
    return to_dev(torch.from_numpy(np.asarray(slots, dtype=np.int64).reshape(-1)), device)


def dev_f32(x, shape, name, device, who):
    """float32 ``shape`` from host, pinned host or device memory -> contiguous on the device, without blocking the host"""
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(np.asarray(x, dtype=np.float32))
    if tuple(x.shape) != shape:
        raise ValueError("%s: %s must be %s (got %s)" % (who, name, shape, tuple(x.shape)))
    if x.dtype != torch.float32:
        raise ValueError("%s: %s must be float32" % (who, name))
    if not x.is_cuda:
        x = to_dev(x, device)
    return x.contiguous()


class SlotState:
    """``S`` slots; once the subclass has checked its arguments, _alloc() makes the first GPU call: ``device``, the state buffer of
    ``nbytes`` bytes and the host counter ``hops[S]``."""

    def __init__(self, streams):
        self.S = int(streams)
        if self.S < 1:
            raise ValueError("%s: streams must be >= 1" % type(self).__name__)

    def _alloc(self, device, nbytes):
        self.device = norm_dev(device)
        self.nbytes = int(nbytes)
        self.state = torch.empty((self.nbytes,), dtype=torch.uint8, device=self.device)
        self.hops = np.zeros(self.S, dtype=np.int64)

    def _slots_mask(self, slots):
        m = np.zeros(self.S, dtype=bool)
        m[np.asarray(slots, dtype=np.int64).reshape(-1)] = True
        return m

    def _flags(self, flags, text):
        return host_flags(flags, self.S, text)

    def _dev_bytes(self, mask):
        return to_dev(torch.from_numpy(mask.astype(np.uint8)), self.device)

    def _dev_f32(self, x, shape, name):
        return dev_f32(x, shape, name, self.device, type(self).__name__)

    def _dev_rows(self, slots):
        return dev_rows(slots, self.device)

    def _out(self, out, shape, dtype=torch.float32, what='out'):
        """the caller's buffer once it has that shape and dtype, or a fresh one on the device"""
        if out is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        if tuple(out.shape) != shape or out.dtype != dtype:
            raise ValueError("%s.process: %s must be %s %s" % (type(self).__name__, what, str(dtype).split('.')[-1], shape))
        return out

    def _hop_args(self, a, b, names, active, out, what='out'):
        """What every hop-wise process() does with its arguments: a, b [S, nh * 256] float32 (host, pinned host or device; ``names`` are
        theirs in the messages), active a host bool sequence [S] or None, out a float32 buffer of that shape or None -> (shape, nh, a
        and b on the device, the host mask or None, its bytes on the device or None, the checked or fresh output)."""
        who = type(self).__name__
        shape = tuple(np.shape(a))
        if len(shape) != 2 or shape[0] != self.S or shape[1] % HOP or shape[1] == 0:
            raise ValueError("%s.process: %s must be [%d, nh * 256]" % (who, names[0], self.S))
        a = self._dev_f32(a, shape, names[0])
        b = self._dev_f32(b, shape, names[1])
        act = None if active is None else self._flags(active, "%s: active must hold one flag per stream" % who)
        return shape, shape[1] // HOP, a, b, act, None if act is None else self._dev_bytes(act), self._out(out, shape, what=what)

    def _count(self, act, nh):
        """the host counter of the slots a call ran in"""
        self.hops[slice(None) if act is None else act] += nh
