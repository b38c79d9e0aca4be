"""Generator / discriminators of NELE-GAN on the MI355X: the host-side mirror of the reference ``model.py``.

Same class names, ``forward`` signatures, shapes and ``state_dict`` keys as the reference
(``Generator_Conv1D_cLN.forward(x[B,T,64], y[B,T,64]) -> [B,T,64]`` model.py:83;
``Discriminator.forward(x[B,3,64,T]) -> [B,3]`` model.py:118; ``Discriminator_Quality`` model.py:152),
so reference checkpoints ('enhance-model' / 'intel-model', train_nele.py:274-277) load unchanged.

The torch ``nn.Module`` objects only OWN the parameters (torch's Conv1d / Conv2d / Linear /
spectral_norm containers are used so that keys, shapes and initialisation match by construction; they
are never called).  Every forward and backward pass runs in libnele_hip.so: implicit-GEMM convolutions
on the f32 matrix cores (csrc/dense.hip), cLN scan, spectral-norm power iteration, pooling + MLP head
(csrc/gen.hip, csrc/disc.hip).  ``torch.autograd.Function`` is the glue that lets the reference's loop
(``loss.backward()``) drive those kernels; parameter gradients are accumulated straight into a flat
gradient buffer (one bucket per model: what Adam and the RCCL all-reduce operate on).
"""
import ctypes
import os

import torch
import torch.nn as nn
from torch.nn.utils import spectral_norm

from . import ops
from . import _lib
from ._lib import c_longlong, c_void_p, call, norm_dev, ptr, stream


# ------------------------------------------------------------------ parameter containers (reference names)
class ConvNorm(nn.Module):
    """model.py:10-28 (parameter container; the convolution itself runs in nele_conv_gemm)."""

    def __init__(self, in_channels, out_channels, kernel_size=1, stride=1, padding=None, dilation=1, bias=True,
                 w_init_gain='linear'):
        super().__init__()
        if padding is None:
            assert kernel_size % 2 == 1
            padding = int(dilation * (kernel_size - 1) / 2)
        self.conv = nn.Conv1d(in_channels, out_channels, kernel_size=kernel_size, stride=stride, padding=padding,
                              dilation=dilation, bias=bias)
        nn.init.xavier_uniform_(self.conv.weight, gain=nn.init.calculate_gain(w_init_gain))


class Chomp1d(nn.Module):
    """model.py:31-40: dropping the right overhang of a conv padded by k-1 == causal left padding."""

    def __init__(self, chomp_size):
        super().__init__()
        self.chomp_size = chomp_size


class cLN(nn.Module):
    """model.py:168-205 (parameter container; the scan runs in nele_cln_fwd / nele_cln_bwd)."""

    def __init__(self, dimension, eps=1e-8, trainable=True):
        super().__init__()
        self.eps = eps
        self.gain0 = nn.Parameter(torch.ones(1, dimension, 1), requires_grad=trainable)
        self.bias0 = nn.Parameter(torch.zeros(1, dimension, 1), requires_grad=trainable)


# precision string -> the library's precision code (NELE_PREC_*): 'bf16' 1, 'bf16x3' 2 (split-operand bf16 products, float32-grade), anything
# else 0 (float32 operands)
_PREC_CODES = {'bf16': 1, 'bf16x3': 2}


def _prec_code(precision):
    return _PREC_CODES.get(precision, 0)


class FlatParams:
    """All parameters of a module as views into ONE flat buffer (+ one flat gradient buffer)."""

    def __init__(self, module):
        self.module = module
        self.flat = None
        self.grad = None
        self._plist = None       # [(parameter, offset)] of the flattened module (ensure() fills it)

    def params(self):
        return [p for p in self.module.parameters()]

    def valid(self, device):
        """True while every parameter (and its gradient) is still the view into the flat buffers that ensure() made.  Checked on every
        forward / prepare (ten times per training step), so it walks the list ensure() kept instead of module.parameters() - the
        recursive enumeration was 75 of this call's 100 us.  Replacing a parameter's storage (.to(), .data = ...) is noticed here;
        ADDING a parameter to a module after its first forward pass is not supported."""
        if self.flat is None or self._plist is None:
            return False
        device = norm_dev(device)
        if self.flat.device != device:
            return False
        f0, g0 = self.flat.data_ptr(), self.grad.data_ptr()
        for p, off in self._plist:
            g = p.grad
            if g is None or p.data_ptr() != f0 + off or g.data_ptr() != g0 + off:
                return False
        return True

    def ensure(self, device):
        device = norm_dev(device)
        if self.valid(device):
            return
        ps = self.params()
        n = sum(p.numel() for p in ps)
        flat = torch.empty(n, dtype=torch.float32, device=device)
        grad = torch.zeros(n, dtype=torch.float32, device=device)
        off = 0
        cur = torch.cuda.current_stream(device) if device.type == 'cuda' else None
        for p in ps:
            k = p.numel()
            flat[off:off + k].copy_(p.data.reshape(-1).to(device))
            if p.grad is not None:
                grad[off:off + k].copy_(p.grad.reshape(-1).to(device))
            # The old storages lose their last reference below and go back to the allocator at once; it only knows the stream they were
            # ALLOCATED on.  If this runs on another stream (D.prepare on a side stream, first step of a fresh trainer) the copies above
            # may still be pending there when the main stream reuses the blocks: round 2 found D's initial weights silently corrupted
            # whenever the side stream lagged.  record_stream makes the allocator wait for this stream too.
            if cur is not None and p.data.is_cuda:
                p.data.record_stream(cur)
                if p.grad is not None and p.grad.is_cuda:
                    p.grad.record_stream(cur)
            p.data = flat[off:off + k].view(p.shape)
            p.grad = grad[off:off + k].view(p.shape)
            off += k
        self.flat, self.grad = flat, grad
        self._plist, off = [], 0
        for p in ps:
            self._plist.append((p, 4 * off))
            off += p.numel()


class _Anchor:
    """A 1-element leaf that requires grad, so autograd calls our backward even when the data
    inputs do not require grad (G-step: clean/noise features are constants)."""

    def __init__(self):
        self.t = None

    def get(self, device):
        device = norm_dev(device)
        if self.t is None or self.t.device != device:
            self.t = torch.zeros(1, device=device, requires_grad=True)
        return self.t


def _empty(shape, dev):
    return torch.empty(shape, dtype=torch.float32, device=dev)


MAX_BUFFER_SHAPES = int(os.environ.get('NELE_MAX_BUFFER_SHAPES', '16'))   # (a corpus of files of many lengths: D batches of ~18 padded shapes; 288 GB of HBM)


class _Workspace:
    """One workspace of the library's plan builders (csrc/netplan.hip) - every activation, weight layout and temporary of one (shape,
    precision, slot, mode) of a module - and the job tables the library built over it."""

    def __init__(self, nbytes, dev, owner):
        self.buf = torch.empty(max(1, int(nbytes)), dtype=torch.uint8, device=dev)
        self.owner = owner                   # the parameter / gradient (/ u, v) pointers the tables were built on
        self.plans = {}                      # form -> plan handle (int)
        self.gen = 0
        self.token = 0
        self.frozen = None                   # G: freeze generation whose weight layouts this workspace holds
        self.din = self.wvalid = self.ddin = None   # D: the last forward pass's input and frame counts, the input gradient's buffer
        self.c16 = False                     # D: bf16 activations in memory

    def add(self, form, handle):
        self.plans[form] = handle.value
        return handle.value

    def reserve_tokens(self, n):
        """n consecutive carry tokens for the fused layer launches of one forward pass; never 0 (zero-initialised slots must not match)"""
        if self.token + n >= 0xFFFFFFF0:
            self.token = 0
        self.token += n
        return self.token - n + 1

    def __del__(self):
        try:
            for h in self.plans.values():
                _lib.lib.nele_plan_destroy(c_void_p(h))
        except Exception:
            pass


def _workspace(module, key, owner, make):
    """The module's workspace of ``key``, least-recently-used bounded: a long run over padded batches of many different shapes (D epochs on a
    real corpus) would otherwise pin one multi-hundred-MB workspace per shape until the process ends.  Tables built on other parameter
    buffers (FlatParams re-homed them) are dropped with their workspace."""
    cache = module._bufs
    ws = cache.pop(key, None)
    if ws is None or ws.owner != owner:
        while len(cache) >= MAX_BUFFER_SHAPES:
            cache.pop(next(iter(cache)))             # dicts keep insertion order: the first key is the least recently used
        ws = make()
    cache[key] = ws                                  # (re-)insert as most recent
    return ws


def _streams(*extra):
    return (c_void_p * (1 + len(extra)))(stream().value, *[s.cuda_stream for s in extra])


def _run_prep(ws, slots=()):
    call('nele_plan_run', c_void_p(ws.plans['prep']), _streams(), 1, (c_longlong * max(1, len(slots)))(*slots), len(slots))


def _check_generation(ctx, name):
    """The activations live in the workspace of their (B, T): a second forward of the same shape overwrites what the first graph's backward
    pass needs.  Each forward bumps the workspace's generation; a backward whose generation is stale raises instead of silently
    differentiating the wrong activations."""
    if ctx.key not in ctx.module._bufs:
        raise RuntimeError("%s: backward() after %d other (batch, frames) shapes went through the module - the cached activations of "
                           "this graph have been evicted (raise NELE_MAX_BUFFER_SHAPES)" % (name, MAX_BUFFER_SHAPES))
    if getattr(ctx, 'precision', None) is not None and ctx.module.precision != ctx.precision:
        raise RuntimeError("%s: `precision` changed from %r to %r between forward() and backward() - the cached activations were written "
                           "for the forward pass's operand type" % (name, ctx.precision, ctx.module.precision))
    if ctx.module._bufs[ctx.key].gen != ctx.gen:
        raise RuntimeError("%s: backward() after another forward pass of the same (batch, frames) shape - the cached activations of "
                           "this graph have been overwritten (run backward before the next forward of that shape)" % name)


# ================================================================== Generator
class _GFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, anchor, module):
        ctx.module = module
        ctx.precision = module.precision
        ctx.key = module._forward_impl(x, y, need_bwd=True)
        ctx.gen = module._bufs[ctx.key].gen
        mask = module._last_mask
        module._last_mask = None             # the output must not stay reachable from ctx except through save_for_backward:
        ctx.save_for_backward(mask)          # output -> grad_fn -> ctx -> output is a cycle the collector cannot free (2 MB per G-step)
        return mask

    @staticmethod
    def backward(ctx, dmask):
        (mask,) = ctx.saved_tensors
        _check_generation(ctx, 'Generator_Conv1D_cLN')
        ctx.module._backward_impl(dmask.contiguous(), ctx.key, mask)
        return None, None, None, None


class Generator_Conv1D_cLN(nn.Module):
    """model.py:43-98."""

    def __init__(self):
        super().__init__()
        self.convolutions = nn.ModuleList()
        self.convolutions.append(nn.Sequential(
            ConvNorm(64 * 2, 256, kernel_size=5, stride=1, padding=int(5 - 1), dilation=1, w_init_gain='tanh'),
            Chomp1d(5 - 1), cLN(256)))
        for _ in range(1, 6 - 1):
            self.convolutions.append(nn.Sequential(
                ConvNorm(256, 256, kernel_size=7, stride=1, padding=int(7 - 1), dilation=1, w_init_gain='tanh'),
                Chomp1d(7 - 1), cLN(256)))
        self.convolutions.append(nn.Sequential(
            ConvNorm(256, 64, kernel_size=5, stride=1, padding=int(5 - 1), dilation=1, w_init_gain='linear'),
            Chomp1d(5 - 1), cLN(64)))
        self.LReLU = nn.LeakyReLU(0.3)
        self.fc1 = nn.Linear(64, 64)
        self.fc2 = nn.Linear(64, 64)
        self._flat = FlatParams(self)
        self._anchor = _Anchor()
        self._bufs = {}                    # (B, T, device, buffer_slot, precision, training pass) -> _Workspace
        self._wstream = None
        self.overlap_wgrad = True          # weight gradients on a second stream beside the data-gradient chain
        self._last_mask = None
        self.precision = 'f32'            # 'bf16': bf16 MFMA operands (f32 accumulate) in the Conv1d / Linear GEMMs (fwd, dgrad, wgrad);
                                          # 'bf16x3': split-operand bf16 products in the Conv1d passes (float32-grade), Linear layers float32
        # Several forward passes in flight on different streams (inference.Enhancer.enhance_stream): each stream names its own workspace
        # through `buffer_slot`.  While the weights are frozen (freeze_weights) a workspace writes its weight layouts once, at its first
        # forward pass, instead of at the head of every forward pass.
        self.buffer_slot = 0
        self._weights_frozen = False
        self._freeze_gen = 0
        # new weights invalidate frozen layouts (inference.Enhancer keeps the layouts of a generator it owns across calls)
        self.register_load_state_dict_post_hook(lambda module, incompatible_keys: module.unfreeze_weights())

    # ---- plumbing
    def train(self, mode=True):
        """The sub-modules are parameter containers that are never called: only this module's own flag means anything, and
        nn.Module.train's walk over the 35 of them cost 0.12 ms per G.eval() / G.train() pair of every generate() call."""
        self.training = bool(mode)
        return self

    def flat_parameters(self, device=None):
        device = device or next(self.parameters()).device
        self._flat.ensure(device)
        return self._flat

    def freeze_weights(self, dev=None):
        """Skip the weight-layout step in the forward passes that follow, until unfreeze_weights(): each workspace writes the layouts of the
        current parameters once, at its first forward pass from now on.  For evaluation loops whose parameters do not change
        (inference.py:79-117): forward passes on several streams then only READ their layouts.  Returns an event recorded on the current
        stream."""
        dev = norm_dev(dev or next(self.parameters()).device)
        self._flat.ensure(dev)
        self._freeze_gen += 1
        self._weights_frozen = True
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        return ev

    def unfreeze_weights(self):
        self._weights_frozen = False

    def _workspace(self, B, T, dev, need_bwd):
        key = (B, T, str(norm_dev(dev)), self.buffer_slot, self.precision, bool(need_bwd))
        fl = self._flat

        def make():
            b16 = _prec_code(self.precision)
            n = _lib.lib.nele_gen_workspace_bytes(B, T, b16, int(need_bwd))
            ws = _Workspace(n, dev, (fl.flat.data_ptr(), fl.grad.data_ptr()))
            prep, fwd = c_void_p(), c_void_p()
            call('nele_gen_plans_build', B, T, b16, int(need_bwd), 0, ptr(fl.flat), ptr(fl.grad), ptr(ws.buf), n, 1, stream(), ctypes.byref(prep),
                 ctypes.byref(fwd), None)
            ws.add('prep', prep)
            ws.add('fwd', fwd)
            return ws
        return key, _workspace(self, key, (fl.flat.data_ptr(), fl.grad.data_ptr()), make)

    # ---- forward (model.py:83-98)
    def _forward_impl(self, x, y, need_bwd=False):
        if x.dim() != 3 or x.shape[2] != 64 or y.shape != x.shape:
            raise ValueError("Generator_Conv1D_cLN.forward: x and y must both be [B, T, 64]")
        if not x.is_cuda:
            raise RuntimeError("nele_gan_amd: the generator runs on the GPU only (no CPU fallback)")
        dev = x.device
        self._flat.ensure(dev)
        B, T, _ = x.shape
        if self._weights_frozen and need_bwd:
            self.unfreeze_weights()           # a pass that will be differentiated: the layouts follow the weights again (an evaluation loop
                                              # freezes them anew)
        key, ws = self._workspace(B, T, dev, need_bwd)
        ws.gen += 1
        xs, ys = x.contiguous().float(), y.contiguous().float()
        mask = _empty((B, T, 64), dev)
        if not self._weights_frozen or ws.frozen != self._freeze_gen:
            _run_prep(ws)
            ws.frozen = self._freeze_gen if self._weights_frozen else None
        call('nele_gen_fwd', c_void_p(ws.plans['fwd']), ptr(xs), ptr(ys), ptr(mask), ws.reserve_tokens(6), _streams(), 1)
        self._last_mask = mask
        return key

    def forward(self, x, y):
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return _GFn.apply(x, y, self._anchor.get(x.device), self)
        self._forward_impl(x, y)
        mask, self._last_mask = self._last_mask, None
        return mask

    # ---- backward: accumulates into the flat gradient buffer
    def _backward_impl(self, dmask, key, mask):
        ws = self._bufs[key]
        B, T = key[0], key[1]
        overlap = bool(self.overlap_wgrad)    # data-gradient chain on the current stream, weight gradients on a second stream beside it
        plan = ws.plans.get(('bwd', overlap))
        if plan is None:
            fl, h = self._flat, c_void_p()
            call('nele_gen_plans_build', B, T, _prec_code(self.precision), 1, int(overlap), ptr(fl.flat), ptr(fl.grad), ptr(ws.buf), ws.buf.numel(), 0,
                 stream(), None, None, ctypes.byref(h))
            plan = ws.add(('bwd', overlap), h)
        side = ()
        if overlap:
            if self._wstream is None:
                self._wstream = ops.side_stream(dmask.device)
            side = (self._wstream,)
        call('nele_gen_bwd', c_void_p(plan), ptr(dmask), ptr(mask), _streams(*side), 1 + len(side))


# ================================================================== Discriminators
_D5_OUT = (64, 3888)                   # conv5: output channels, reduction length 48 * 9 * 9 (the launches ops.PROFILE times)


class _DFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, din, anchor, module, frames=None):
        ctx.module = module
        ctx.precision = module.precision
        ctx.key = module._forward_impl(din, frames)
        ctx.wvalid = module._bufs[ctx.key].wvalid
        ctx.gen = module._bufs[ctx.key].gen
        ctx.need_din = din.requires_grad
        score = module._last_score
        module._last_score = None
        ctx.save_for_backward(score)
        return score

    @staticmethod
    def backward(ctx, dscore):
        (score,) = ctx.saved_tensors
        _check_generation(ctx, 'Discriminator')
        ddin = ctx.module._backward_impl(dscore.contiguous(), ctx.key, ctx.need_din, score, ctx.wvalid)
        return ddin, None, None, None


class _NchwToPacked(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.cin = x.shape[1]
        return ops.nchw_to_nhwc4(x.float())

    @staticmethod
    def backward(ctx, ddin):
        return ops.nhwc4_to_nchw(ddin.contiguous(), ctx.cin)


def _profiled(name, libtag):
    """ops.PROFILE's list ``name`` with the library's hook armed for ``libtag`` (beside whatever else is armed), or None."""
    lst = ops.PROFILE.get(name) if ops.PROFILE is not None else None
    if lst is not None:
        _lib.profile_begin('+' + libtag)
    return lst


def _collect(lst, libtag, work):
    if lst is not None:
        lst.extend((ops.Ms(0.0), ops.Ms(ms), work) for ms in _lib.profile_collect_tag(libtag))


class _DiscriminatorBase(nn.Module):
    def __init__(self, cin, nout):
        super().__init__()
        self._cin, self._nout = cin, nout
        layers = [spectral_norm(nn.Conv2d(cin, 8, (1, 1))),
                  spectral_norm(nn.Conv2d(8, 16, (3, 3))),
                  spectral_norm(nn.Conv2d(16, 32, (5, 5))),
                  spectral_norm(nn.Conv2d(32, 48, (7, 7))),
                  spectral_norm(nn.Conv2d(48, 64, (9, 9)))]
        self.layers = nn.ModuleList(layers)
        self.GAPool = nn.AdaptiveAvgPool2d((1, 1))
        self.LReLU = nn.LeakyReLU(0.3)
        self.fc1 = spectral_norm(nn.Linear(64, 64))
        self.fc2 = spectral_norm(nn.Linear(64, 16))
        self.fc3 = spectral_norm(nn.Linear(16, nout))
        self._flat = FlatParams(self)
        self._anchor = _Anchor()
        self._bufs = {}                    # (B, T, device, precision) -> _Workspace
        self._sigma = None
        self._last_score = None
        self._prepared = None
        self._wstream = None
        self.overlap_wgrad = True          # weight gradients on two more streams beside the data-gradient chain
        self.profile_prefix = ''           # prepended to the ops.PROFILE name of this module's conv5 forward launches (bench.py)
        self.weight_grad_enabled = True   # reference computes (unused) D weight grads in the G-step too
        self.precision = 'f32'            # 'bf16': bf16 MFMA operands (f32 accumulate) in the conv forward / data-gradient passes;
                                          # 'bf16x3': split-operand bf16 products in the k > 1 conv passes (float32-grade)

    def flat_parameters(self, device=None):
        device = device or next(self.parameters()).device
        self._flat.ensure(device)
        return self._flat

    def _sn_modules(self):
        return list(self.layers) + [self.fc1, self.fc2, self.fc3]

    def train(self, mode=True):
        """see Generator_Conv1D_cLN.train (the spectral-norm hooks of the sub-modules never run: the power iteration is nele_spectral_norm)"""
        self.training = bool(mode)
        return self

    def sn_uv_host(self):
        """(weight_u, weight_v) device pointers of the 8 spectral-norm layers, in the order of the flat parameters"""
        return (c_void_p * 16)(*[t.data_ptr() for m in self._sn_modules() for t in (m.weight_u, m.weight_v)])

    def _workspace(self, B, T, dev):
        key = (B, T, str(norm_dev(dev)), self.precision)
        fl = self._flat
        uv = self.sn_uv_host()
        owner = (fl.flat.data_ptr(), fl.grad.data_ptr()) + tuple(uv)

        def make():
            b16 = _prec_code(self.precision)
            n = _lib.lib.nele_disc_workspace_bytes(B, T, self._cin, b16)
            if n < 0:
                raise ValueError("Discriminator: T=%d is too short (needs T >= 21, model.py:105-109)" % T)
            ws = _Workspace(n, dev, owner)
            prep, fwd = c_void_p(), c_void_p()
            call('nele_disc_plans_build', B, T, self._cin, self._nout, b16, 0, 0, 0, ptr(fl.flat), ptr(fl.grad), uv, ptr(ws.buf), n, 1, stream(),
                 ctypes.byref(prep), ctypes.byref(fwd), None)
            ws.add('prep', prep)
            ws.add('fwd', fwd)
            off = _lib.lib.nele_disc_workspace_ddin(ptr(ws.buf), B, T, self._cin, b16) - ws.buf.data_ptr()
            ws.ddin = ws.buf[off:off + B * 64 * T * 4 * 4].view(torch.float32).view(B, 64, T, 4)
            es = ctypes.c_int(0)                             # activations stored as bfloat16 (csrc/conv16.hip) where every layer allows it
            ws.c16 = bool(_lib.lib.nele_disc_workspace_buffer(ptr(ws.buf), B, T, self._cin, b16, b'act1', ctypes.byref(es))) and es.value == 2
            return ws
        return key, _workspace(self, key, owner, make)

    def prepare(self, B, T, dev):
        """Spectral-norm power iteration + sigma (model.py:105-116) and every weight layout of a forward / backward pass at batch B,
        frames T, enqueued on the CURRENT stream.  The next forward of that shape waits for it instead of doing it inline:
        this work only depends on the parameters, so a training loop can run it on another stream ahead of the forward pass
        (GanTrainer does, beside the generator's forward pass and beside generate)."""
        self._flat.ensure(dev)
        key, ws = self._workspace(B, T, dev)
        _run_prep(ws, (int(self.training),))
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        self._prepared = (key, self.training, ev)

    def advance_power_iteration(self, dev=None):
        """One spectral-norm power iteration of every layer (what a training-mode forward pass does first, model.py:105-116), no data.
        An empty data-parallel step (this rank has run out of batches) calls it so that weight_u / weight_v advance in lock-step with
        the ranks that ran a real forward pass: all replicas then normalise by the same sigma and rank 0's checkpoint is what a
        single-GPU run of the same steps would hold."""
        if not self.training:
            return
        dev = norm_dev(dev or next(self.parameters()).device)
        self._flat.ensure(dev)
        if self._sigma is None or self._sigma.device != dev:
            self._sigma = torch.zeros(8, device=dev)         # (every forward pass computes its own sigma again)
        mods = self._sn_modules()
        pp = (c_void_p * (3 * len(mods)))()
        dd = (ctypes.c_int * (2 * len(mods)))()
        for i, m in enumerate(mods):
            pp[3 * i], pp[3 * i + 1], pp[3 * i + 2] = m.weight_orig.data_ptr(), m.weight_u.data_ptr(), m.weight_v.data_ptr()
            dd[2 * i] = m.weight_orig.shape[0]
            dd[2 * i + 1] = m.weight_orig.numel() // m.weight_orig.shape[0]
        call('nele_spectral_norm', pp, dd, len(mods), ptr(self._sigma), 1, stream())

    def _forward_impl(self, din, frames=None):
        if not din.is_cuda:
            raise RuntimeError("nele_gan_amd: the discriminator runs on the GPU only (no CPU fallback)")
        dev = din.device
        self._flat.ensure(dev)
        B, H, T, C4 = din.shape
        assert H == 64 and C4 == 4
        key, ws = self._workspace(B, T, dev)
        prep, self._prepared = self._prepared, None
        if prep is not None and prep[1] == self.training:
            torch.cuda.current_stream().wait_event(prep[2])
            if prep[0] != key:
                # prepared for another shape: u, v have already advanced once for this forward pass (the reference advances them once per
                # training forward, model.py:105-116) - only the shape-dependent weight layouts are redone
                _run_prep(ws, (0,))
        else:
            _run_prep(ws, (int(self.training),))
        ws.gen += 1
        a = din.contiguous()
        ws.din = a
        score = _empty((B, self._nout), dev)
        # padded batch of utterances of different lengths: the pooling runs over each utterance's own valid output columns (frames - 20)
        ws.wvalid = None if frames is None else (frames.to(device=dev, dtype=torch.int32) - 20).contiguous()
        # the kernel that runs D.conv5's forward: the span kernel (float32), the split tile kernel (bf16x3), conv16 (bf16)
        libtag = {'bf16': 'conv16_N%d_K%d_e2', 'bf16x3': 'tile16x3_N%d_K%d'}.get(self.precision, 'span_N%d_K%d') % _D5_OUT
        prof = _profiled(self.profile_prefix + 'D.conv5.fwd', libtag)
        call('nele_disc_fwd', c_void_p(ws.plans['fwd']), ptr(a), ptr(ws.wvalid), ptr(score), _streams(), 1)
        _collect(prof, libtag, 2.0 * B * 44 * (T - 20) * _D5_OUT[0] * _D5_OUT[1])
        self._last_score = score
        return key

    def forward_packed(self, din, frames=None):
        """din: channels-last [B,64,T,4] (ops.d_pack / energy-norm output).  frames [B] (optional): STFT frames of each utterance
        inside a padded batch (every utterance needs >= 21, like T)."""
        if torch.is_grad_enabled() and (din.requires_grad or any(p.requires_grad for p in self.parameters())):
            return _DFn.apply(din, self._anchor.get(din.device), self, frames)
        self._forward_impl(din, frames)
        score, self._last_score = self._last_score, None
        return score

    def forward(self, x):
        """x: [B, Cin, 64, T] as in the reference (model.py:118)."""
        if x.dim() != 4 or x.shape[1] != self._cin or x.shape[2] != 64:
            raise ValueError("%s.forward: x must be [B, %d, 64, T]" % (type(self).__name__, self._cin))
        return self.forward_packed(_NchwToPacked.apply(x))

    def _backward_impl(self, dscore, key, need_din, score, wvalid=None):
        ws = self._bufs[key]
        B, T = key[0], key[1]
        wgrad = bool(self.weight_grad_enabled)
        # The data-gradient chain (layer l's needs layer l+1's) stays on the current stream; a layer's weight gradient (+ its spectral-norm
        # chain rule and bias gradient) only needs that layer's output gradient, so those run on two more streams beside the chain and join
        # at the end.  In the D-step this tail is fully exposed (nothing else is left to overlap).
        overlap = wgrad and bool(self.overlap_wgrad)
        form = ('bwd', bool(need_din), wgrad, overlap)
        plan = ws.plans.get(form)
        if plan is None:                      # another backward form over the same workspace: built without zeroing it again
            fl, h = self._flat, c_void_p()
            call('nele_disc_plans_build', B, T, self._cin, self._nout, _prec_code(self.precision), int(need_din), int(wgrad), int(overlap), ptr(fl.flat),
                 ptr(fl.grad), self.sn_uv_host(), ptr(ws.buf), ws.buf.numel(), 0, stream(), None, None, ctypes.byref(h))
            plan = ws.add(form, h)
        side = ()
        if overlap:
            if self._wstream is None:
                self._wstream = (ops.side_stream(dscore.device), ops.side_stream(dscore.device))
            side = self._wstream
        libtag = 'wgrad_N%d_K%d' % _D5_OUT
        prof = _profiled('D.conv5.wgrad', libtag) if wgrad else None
        call('nele_disc_bwd', c_void_p(plan), ptr(dscore), ptr(score), ptr(wvalid), ptr(ws.din), _streams(*side), 1 + len(side))
        # algorithmic bytes: the input and the output gradient read once (float32), the weight gradient written once
        _collect(prof, libtag, 4.0 * (B * 52 * (T - 12) * 48 + B * 44 * (T - 20) * _D5_OUT[0] + _D5_OUT[0] * _D5_OUT[1]))
        return ws.ddin if need_din else None


class Discriminator(_DiscriminatorBase):
    """model.py:101-132: input channels (enhanced, noise, clean); outputs (SIIB, HASPI, ESTOI) scores.
    ``nout`` is configurable (build-side feature) for metric subsets, e.g. 2 for SIIB+ESTOI."""

    def __init__(self, nout=3):
        super().__init__(3, nout)


class Discriminator_Quality(_DiscriminatorBase):
    """model.py:135-166: input channels (enhanced, clean); outputs (PESQ, ViSQOL) scores."""

    def __init__(self, nout=2):
        super().__init__(2, nout)


# ================================================================== energy normalisation glue (train_nele.py:133-146)
class _EnergyNormPack(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mask, clean, noise, p, inv_p):
        beta2, s2, din, _ = ops.energy_norm_fwd(clean, mask, noise, p, inv_p, want_din=True)
        ctx.save_for_backward(mask, clean, beta2, s2, din)
        ctx.p, ctx.inv_p = p, inv_p
        ctx.mark_non_differentiable(beta2)
        return din, beta2

    @staticmethod
    def backward(ctx, ddin, dbeta2):
        mask, clean, beta2, s2, din = ctx.saved_tensors
        dmask = ops.energy_norm_bwd(clean, mask, beta2, s2, ddin.contiguous(), ctx.p, ctx.inv_p, din=din)
        return dmask, None, None, None, None


class _EnergyNormPackPrefix(torch.autograd.Function):
    """The causal (prefix) form: every frame normalised by the energy sums of the frames up to it (nele_energy_norm_prefix_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, mask, clean, noise, p, inv_p):
        ratio, s2, din, _ = ops.energy_norm_prefix_fwd(clean, mask, noise, p, inv_p, want_din=True)
        ctx.save_for_backward(mask, clean, ratio, s2, din)
        ctx.p, ctx.inv_p = p, inv_p
        ctx.mark_non_differentiable(ratio)
        return din, ratio

    @staticmethod
    def backward(ctx, ddin, dratio):
        mask, clean, ratio, s2, din = ctx.saved_tensors
        dmask = ops.energy_norm_prefix_bwd(clean, mask, ratio, s2, ddin.contiguous(), ctx.p, ctx.inv_p, din=din)
        return dmask, None, None, None, None


NORMS = ('utterance', 'prefix')


def check_norm(norm, who):
    """'utterance': the reference's sums over the whole utterance (train_nele.py:133-140); 'prefix': sums over the frames up to each
    frame - causal, what realtime.RealtimeEnhancer emits."""
    if norm not in NORMS:
        raise ValueError("%s: norm must be 'utterance' or 'prefix' (got %r)" % (who, norm))
    return norm


def energy_norm_pack(mask, clean_band, noise_band, p_power=1.0 / 6, inv_p=6.0, norm='utterance'):
    """mask, clean_band, noise_band [B,T,64] -> (D input [B,64,T,4] = (enh, noise, clean, 0), beta2 [B]).
    Utterance-level (per sample) normalisation, as the batch-1 reference (train_nele.py:133-146).
    norm='prefix': the causal form of the real-time path; the second value is then ratio [B,T] (beta2 of every prefix)."""
    fn = _EnergyNormPackPrefix if check_norm(norm, 'energy_norm_pack') == 'prefix' else _EnergyNormPack
    return fn.apply(mask.contiguous(), clean_band.contiguous(), noise_band.contiguous(), float(p_power), float(inv_p))


def normed_alpha2(mask, clean_band, inv_p=6.0, frames=None, norm='utterance'):
    """mask * beta_2 (train_nele.py:303-307; inference.py:99-104), no autograd.  frames [B]: STFT frames of each utterance inside a
    padded batch (the energy sums of beta_2 run over those frames only).
    norm='prefix': mask[t] * ratio[t], bit-identical to the real-time path's alpha^2 on bit-equal band features and mask."""
    if check_norm(norm, 'normed_alpha2') == 'prefix':
        return ops.energy_norm_prefix_fwd(clean_band.contiguous(), mask.contiguous(), None, 1.0 / inv_p, float(inv_p), want_din=False,
                                          want_alpha2=True)[3]
    _, _, _, alpha2 = ops.energy_norm_fwd(clean_band.contiguous(), mask.contiguous(), None, 1.0 / inv_p, float(inv_p), want_din=False,
                                          want_alpha2=True, frames=frames)
    return alpha2
