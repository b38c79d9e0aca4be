"""ctypes binding of libnele_hip.so (the C ABI of include/nele_hip.h and, for the entry points added after its fixed set,
include/nele_hip_ext.h, after that one's, include/nele_hip_ext2.h, after that one's, include/nele_hip_ext3.h, after that one's, include/nele_hip_ext4.h, after that one's, include/nele_hip_ext5.h, after that one's, include/nele_hip_ext6.h, after that one's, include/nele_hip_ext7.h, after that one's, include/nele_hip_ext8.h, after that one's, include/nele_hip_ext9.h and, after that one's, include/nele_hip_ext10.h).

The HIP library IS the product path: if it is missing or fails to load this module raises; there
is no CPU or eager-PyTorch fallback anywhere in the package.
"""
import ctypes
import os

import torch

from . import _abi, _abi_ext, _abi_ext2, _abi_ext3, _abi_ext4, _abi_ext5, _abi_ext6, _abi_ext7, _abi_ext8, _abi_ext9, _abi_ext10

FUNCS = dict(_abi.FUNCS, **_abi_ext.FUNCS)          # name -> (restype, argtypes) of the two headers
CONSTS = dict(_abi.CONSTS, **_abi_ext.CONSTS)
FUNCS2 = dict(_abi_ext2.FUNCS)                      # the third header's, in dicts of their own: the two above keep their sizes
CONSTS2 = dict(_abi_ext2.CONSTS)
FUNCS3 = dict(_abi_ext3.FUNCS)                      # the fourth header's, likewise; their argtypes are in _SIGS3
CONSTS3 = dict(_abi_ext3.CONSTS)
FUNCS4 = dict(_abi_ext4.FUNCS)                      # the fifth header's, likewise; their argtypes are in _SIGS4
CONSTS4 = dict(_abi_ext4.CONSTS)
FUNCS5 = dict(_abi_ext5.FUNCS)                      # the sixth header's, likewise; their argtypes are in _SIGS5
CONSTS5 = dict(_abi_ext5.CONSTS)
FUNCS6 = dict(_abi_ext6.FUNCS)                      # the seventh header's, likewise; their argtypes are in _SIGS6
CONSTS6 = dict(_abi_ext6.CONSTS)
FUNCS7 = dict(_abi_ext7.FUNCS)                      # the eighth header's, likewise; their argtypes are in _SIGS7
CONSTS7 = dict(_abi_ext7.CONSTS)
FUNCS8 = dict(_abi_ext8.FUNCS)                      # the ninth header's, likewise; their argtypes are in _SIGS8
CONSTS8 = dict(_abi_ext8.CONSTS)
FUNCS9 = dict(_abi_ext9.FUNCS)                      # the tenth header's, likewise; their argtypes are in _SIGS9
CONSTS9 = dict(_abi_ext9.CONSTS)
FUNCS10 = dict(_abi_ext10.FUNCS)                    # the eleventh header's, likewise; their argtypes are in _SIGS10
CONSTS10 = dict(_abi_ext10.CONSTS)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('NELE_LIB') or os.path.join(_HERE, 'libnele_hip.so')     # NELE_LIB: another build of the same ABI (A/B measurements)

c_int = ctypes.c_int
c_float = ctypes.c_float
c_double = ctypes.c_double
c_void_p = ctypes.c_void_p
c_size_t = ctypes.c_size_t
c_longlong = ctypes.c_longlong


class NeleError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "nele_gan_amd: %s not found -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C nele_gan_amd/csrc` (hipcc, gfx950). There is no fallback path." % LIB_PATH)
    return ctypes.CDLL(LIB_PATH)


lib = _load()


def _bind(every):
    """Sets argtypes and restype of the entry points ``every`` (_abi*.FUNCS, generated from include/nele_hip.h, nele_hip_ext.h,
    nele_hip_ext2.h, nele_hip_ext3.h, nele_hip_ext4.h, nele_hip_ext5.h, nele_hip_ext6.h, nele_hip_ext7.h, nele_hip_ext8.h, nele_hip_ext9.h and nele_hip_ext10.h by tools/gen_abi.py) -> name -> argtypes."""
    missing = sorted(n for n in every if not hasattr(lib, n))
    if missing:
        raise ImportError("nele_gan_amd: %s does not export %s (declared in include/nele_hip*.h) -- "
                          "rebuild it with `python -c 'import __graft_entry__ as g; g.build()'`" % (LIB_PATH, ', '.join(missing)))
    sigs = {}
    for name, (restype, argtypes) in every.items():
        fn = getattr(lib, name)
        fn.restype = getattr(ctypes, 'c_' + restype)
        fn.argtypes = sigs[name] = [getattr(ctypes, 'c_' + a) for a in argtypes]
    return sigs


_SIGS = _bind(dict(FUNCS, **FUNCS2))
_SIGS3 = _bind(FUNCS3)
_SIGS4 = _bind(FUNCS4)
_SIGS5 = _bind(FUNCS5)
_SIGS6 = _bind(FUNCS6)
_SIGS7 = _bind(FUNCS7)
_SIGS8 = _bind(FUNCS8)
_SIGS9 = _bind(FUNCS9)
_SIGS10 = _bind(FUNCS10)


def check(status, name=''):
    if status != 0:
        msg = lib.nele_last_error_string().decode('utf-8', 'replace')
        if status == -1:
            raise ValueError("%s: %s" % (name, msg))
        raise NeleError("%s failed (status %d): %s" % (name, status, msg))


# ------------------------------------------------------------------ job tables (csrc/plan.hip): the generic form of a plan's jobs
PLAN_MAXARGS = CONSTS['NELE_PLAN_MAXARGS']


class nele_plan_job(ctypes.Structure):
    _fields_ = [('op', c_int), ('nargs', c_int), ('stream', c_int), ('slot', c_int * PLAN_MAXARGS), ('ival', c_longlong * PLAN_MAXARGS),
                ('fval', c_double * PLAN_MAXARGS)]


def call(name, *args):
    check(getattr(lib, name)(*args), name)


def ptr(t):
    """Device pointer of a contiguous CUDA(HIP) tensor, or NULL for None."""
    if t is None:
        return None
    if not t.is_cuda:
        raise ValueError("nele_gan_amd: expected a tensor on the GPU (got %s)" % t.device)
    if not t.is_contiguous():
        raise ValueError("nele_gan_amd: expected a contiguous tensor")
    return c_void_p(t.data_ptr())


def norm_dev(dev):
    """torch.device('cuda') != torch.device('cuda:0'): an index-less device would make every cache keyed by a device look stale (and
    re-home model.FlatParams' buffer on every call).  Normalise to the indexed device."""
    dev = torch.device(dev)
    if dev.type == 'cuda' and dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    return dev


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)
_raw_device = getattr(torch._C, '_cuda_getDevice', None)


def stream():
    """The current torch HIP stream as a hipStream_t.  (torch.cuda.current_stream() builds a Stream object through three Python layers:
    10 us a call, 0.5 ms of a B = 32 step's 4 ms of host time; the raw accessor is the same lookup without the object.)"""
    if _raw_stream is not None and _raw_device is not None:
        return c_void_p(_raw_stream(_raw_device()))
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def profile_begin(tag):
    """Arm the library's HIP-event hook for the launch sites tagged ``tag`` (a name or a comma-separated list; None disarms; a leading
    '+' arms the listed tags beside the armed ones, each with an empty list again)."""
    lib.nele_profile_begin(tag.encode() if tag else None)


def profile_collect_tag(tag, max_n=8192):
    """-> list of durations (ms) of the launches tagged ``tag`` since profile_begin (synchronises on them; the hook stays armed)."""
    buf = (c_float * max_n)()
    n = lib.nele_profile_collect_tag(tag.encode(), buf, max_n)
    return [float(buf[i]) for i in range(n)]


def profile_collect(max_n=4096):
    """-> list of durations (ms) of the tagged launches since profile_begin (synchronises on them)."""
    buf = (c_float * max_n)()
    n = lib.nele_profile_collect(buf, max_n)
    return [float(buf[i]) for i in range(n)]


def device_info():
    cu = c_int(0)
    ws = c_int(0)
    buf = ctypes.create_string_buffer(64)
    call('nele_device_info', ctypes.byref(cu), ctypes.byref(ws), buf, 64)
    return {'cu_count': cu.value, 'wave_size': ws.value, 'arch': buf.value.decode()}
