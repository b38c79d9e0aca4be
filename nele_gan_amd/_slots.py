"""Host side of the per-stream slot state (csrc/slot_state.h): what ``RealtimeEnhancer``, ``EchoCanceller`` and ``StreamResampler`` share -
the slot count, the device, the hop counters, and the ways their arguments reach the device without blocking the host.  Messages carry
the name of the class that raises them."""
import numpy as np
import torch

from ._lib import norm_dev


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
