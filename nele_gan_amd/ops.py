"""Thin Python wrappers over the dense / glue entry points of libnele_hip.so (no arithmetic here)."""
import os

import torch

from . import _lib
from ._lib import c_int, c_longlong, c_void_p, call, ptr, stream


def side_stream(device):
    """A new side stream - or, with NELE_SERIAL=1 (diagnostic: every kernel then runs alone and a rocprofv3 kernel trace shows
    isolated durations), the current stream itself, which serialises the whole step.
    (CU-masked streams - hipExtStreamCreateWithCUMask, to keep the metric streams off part of the GPU - were tried in rounds 1 and 2: a
    masked queue's kernels stop overlapping with the other queues altogether: 96-128 ms per B = 256 step against 78.)"""
    if os.environ.get('NELE_SERIAL', '0') == '1':
        return torch.cuda.current_stream(device)
    return torch.cuda.Stream(device=device)


_probe_warm = False


def shares_queue(a, b, device, spin_us=300.0):
    """Does a kernel on stream ``b`` wait behind a kernel running on stream ``a`` - do the two sit on the same hardware queue?  (The HIP
    runtime multiplexes all streams onto four hardware queues - the default stream's and three for the side streams, assigned at
    creation; streams on one queue run in submission order, whatever their events say.)  Parks one idle wave on ``a`` for ``spin_us`` and
    times a trivial kernel on ``b``: on another queue it finishes long before the spin does.  Asked in BOTH directions (the first probe
    of a process misreads one of them - first kernel launches - and streams that do share a queue wait for each other either way).
    Synchronises the device a few times: for set-up code, once per object."""
    global _probe_warm
    t = torch.zeros(64, device=device)

    def probe(p, q):
        torch.cuda.synchronize(device)
        ea, eb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(p):
            _lib.lib.nele_stream_spin(float(spin_us), c_void_p(p.cuda_stream))
            ea.record(p)
        with torch.cuda.stream(q):
            t.add_(1.0)
            eb.record(q)
        torch.cuda.synchronize(device)
        return eb.elapsed_time(ea) < 0.5 * spin_us * 1e-3       # q's kernel ended less than half a spin before the spin did (or after it)
    if not _probe_warm:
        _probe_warm = True
        probe(a, b)                                             # first launches of both kernels: result discarded
    return probe(a, b) and probe(b, a)


def streams_on_distinct_queues(device, n, have=()):
    """``n`` (at most three) side streams on pairwise different hardware queues, none of them the queue of a stream in ``have``."""
    if os.environ.get('NELE_SERIAL', '0') == '1' or torch.cuda.is_current_stream_capturing():
        return [side_stream(device) for _ in range(n)]
    out = []
    for _ in range(n):
        st, tries = torch.cuda.Stream(device=device), 0
        while tries < 8 and any(shares_queue(o, st, device) for o in list(have) + out):
            st, tries = torch.cuda.Stream(device=device), tries + 1
        out.append(st)
    return out


# bench.py sets PROFILE = {tag: [], ...} to time single launches of the discriminator in float32 mode: while it is set, every forward pass
# of a discriminator appends (start, end, work) for its conv5 launch to PROFILE[profile_prefix + 'D.conv5.fwd'] and every backward pass
# for conv5's weight gradient to PROFILE['D.conv5.wgrad'], when those lists exist; start.elapsed_time(end) is the launch's duration in ms
# (the library's HIP-event hook, collected - synchronising - right after the pass).
PROFILE = None


class Ms:
    """A measured duration with torch.cuda.Event's interface: Ms(0).elapsed_time(Ms(ms)) == ms."""

    def __init__(self, ms):
        self.ms = ms

    def elapsed_time(self, other):
        return other.ms


def glayer16_supported(cin, cout, k):
    """Does the fused layer kernel (conv + bias + cLN + LeakyReLU on bf16 activations, csrc/glayer.hip) take this Conv1d?"""
    return bool(_lib.lib.nele_glayer16_supported(cin, cout, k))


def glayer16_wfrag_elems(cin, cout, k):
    return int(_lib.lib.nele_glayer16_wfrag_elems(cin, cout, k))

def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, guard=None):
    if guard is not None:
        call('nele_adam_step_guarded', ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, beta1, beta2, eps, step, ptr(guard), stream())
    else:
        call('nele_adam_step', ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, beta1, beta2, eps, step, stream())


def energy_norm_fwd(clean, mask, noise, p, inv_p, want_din=True, want_alpha2=False, frames=None):
    """frames [B] is accepted for symmetry with the other padded-batch entry points and needs no kernel support: the band features of
    frames behind an utterance's end are exactly zero (nele_stft_band_var / nele_imcra_band_var), so they add nothing to beta_2's sums,
    their D input is zero and their mask gradient is zero."""
    B, T, _ = clean.shape
    dev = clean.device
    beta2 = torch.empty(B, device=dev)
    s2 = torch.empty(B, device=dev)
    din = torch.empty((B, 64, T, 4), device=dev) if want_din else None
    alpha2 = torch.empty((B, T, 64), device=dev) if want_alpha2 else None
    call('nele_energy_norm_fwd', ptr(clean), ptr(mask), ptr(noise), p, inv_p, ptr(beta2), ptr(s2), ptr(din), ptr(alpha2), B, T, stream())
    return beta2, s2, din, alpha2


def energy_norm_bwd(clean, mask, beta2, s2, ddin, p, inv_p, din=None):
    B, T, _ = clean.shape
    dmask = torch.empty_like(mask)
    call('nele_energy_norm_bwd', ptr(clean), ptr(mask), ptr(beta2), ptr(s2), ptr(ddin), ptr(din), p, inv_p, ptr(dmask), B, T, stream())
    return dmask


def energy_norm_prefix_fwd(clean, mask, noise, p, inv_p, want_din=True, want_alpha2=False):
    """The causal (prefix) form of energy_norm_fwd (csrc/prefixnorm.hip): -> (ratio [B,T] float32, s2 [B,T] float64, din, alpha2).
    Padded batches need no frame counts, for the reason given in energy_norm_fwd."""
    B, T, _ = clean.shape
    dev = clean.device
    ratio = torch.empty((B, T), device=dev)
    s2 = torch.empty((B, T), dtype=torch.float64, device=dev)
    din = torch.empty((B, 64, T, 4), device=dev) if want_din else None
    alpha2 = torch.empty((B, T, 64), device=dev) if want_alpha2 else None
    call('nele_energy_norm_prefix_fwd', ptr(clean), ptr(mask), ptr(noise), p, inv_p, ptr(ratio), ptr(s2), ptr(din), ptr(alpha2), B, T, stream())
    return ratio, s2, din, alpha2


def energy_norm_prefix_bwd(clean, mask, ratio, s2, ddin, p, inv_p, din=None):
    B, T, _ = clean.shape
    dmask = torch.empty_like(mask)
    call('nele_energy_norm_prefix_bwd', ptr(clean), ptr(mask), ptr(ratio), ptr(s2), ptr(ddin), ptr(din), p, inv_p, ptr(dmask), B, T, stream())
    return dmask


def d_pack(c0, c1, c2=None):
    """three (two) band-feature tensors [B,T,64] -> channels-last D input [B,64,T,4] (dataloader.py:76-84)."""
    B, T, _ = c0.shape
    din = torch.empty((B, 64, T, 4), device=c0.device)
    call('nele_d_pack', ptr(c0.contiguous()), ptr(c1.contiguous()), ptr(c2.contiguous() if c2 is not None else None), ptr(din), B, T,
         stream())
    return din


def d_gather(items, rows, Tm, want_frames=True):
    """A list of per-utterance D items [64, T_k, 4] (float32, device; contiguous or rows of a larger padded batch: band rows
    item.stride(0) floats apart) -> (din [rows, 64, Tm, 4] zero-padded, frames [rows] int32 or None): one launch per 64 items
    (nele_d_gather_items) instead of one copy per item."""
    n = len(items)
    dev = items[0].device
    Ts = [int(t.shape[1]) for t in items]
    for t in items:
        if t.dtype != torch.float32 or t.dim() != 3 or t.shape[0] != 64 or t.shape[2] != 4 or t.stride(2) != 1 or t.stride(1) != 4:
            raise ValueError('d_gather: items must be float32 [64, T, 4] with contiguous (T, 4) rows')
    din = torch.empty((rows, 64, Tm, 4), device=dev)
    frames = torch.empty((rows,), dtype=torch.int32, device=dev) if want_frames else None
    pa = (c_void_p * n)(*[t.data_ptr() for t in items])
    fa = (c_int * n)(*Ts)
    sa = (c_longlong * n)(*[int(t.stride(0)) for t in items])
    call('nele_d_gather_items', pa, fa, sa, n, rows, Tm, ptr(din), ptr(frames), stream())
    return din, frames


def nchw_to_nhwc4(x):
    B, Cin, H, T = x.shape
    assert H == 64
    din = torch.empty((B, 64, T, 4), device=x.device)
    call('nele_d_layout', ptr(x.contiguous()), ptr(din), B, Cin, T, 1, stream())
    return din


def nhwc4_to_nchw(ddin, Cin):
    B, H, T, _ = ddin.shape
    dx = torch.empty((B, Cin, 64, T), device=ddin.device)
    call('nele_d_layout', ptr(ddin), ptr(dx), B, Cin, T, 0, stream())
    return dx
