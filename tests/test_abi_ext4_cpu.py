"""CPU: the fifth header include/nele_hip_ext4.h as a whole - it declares exactly the five entry points of the noise suppressor and
none of an earlier header's, both libraries export them, nele_gan_amd/_lib.py binds them with the header's arity and constants in dicts
of their own (the earlier headers' dicts and _SIGS keep their sizes), and tools/gen_abi.py --check notices a stale _abi_ext4.py - and,
in a tree without the fifth header, writes and checks what it did before.  Then the entry points themselves without a GPU: the
state-size arithmetic, bad arguments rejected with the function's name, and NoiseSuppressor's own argument checks."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LL = ctypes.c_longlong
ENTRY_POINTS = ('nele_ns_state_bytes', 'nele_ns_stream_record_bytes', 'nele_ns_init', 'nele_ns_reset', 'nele_ns_hop')
EARLIER_HEADERS = ('nele_hip.h', 'nele_hip_ext.h', 'nele_hip_ext2.h', 'nele_hip_ext3.h')
EARLIER = ('nele_gan_amd/_abi.py', 'nele_gan_amd/_abi_ext.py', 'nele_gan_amd/_abi_ext2.py', 'nele_gan_amd/_abi_ext3.py',
           'nele_gan_amd/csrc/plan_ops.inc')
FIFTH = 'nele_gan_amd/_abi_ext4.py'


def _gen_abi():
    spec = importlib.util.spec_from_file_location('gen_abi', os.path.join(ROOT, 'tools', 'gen_abi.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _header(name='nele_hip_ext4.h'):
    return open(os.path.join(ROOT, 'include', name)).read()


def test_the_fifth_header_declares_the_five_entry_points_and_none_of_an_earlier_header():
    gen = _gen_abi()
    src = _header()
    protos = {p[0]: p for p in gen.prototypes(src)}                              # (raises unless every nele_* name is read as one prototype)
    assert sorted(protos) == sorted(ENTRY_POINTS) and len(set(ENTRY_POINTS)) == 5
    consts = gen.consts(src)
    assert consts == {'NELE_NS_EPS': 1e-10, 'NELE_NS_NU_MIN': 1e-8}
    assert protos['nele_ns_hop'][3] == ['state', 'state_bytes', 'max_streams', 'x', 'active', 'nh', 'gmin', 'out', 'gains', 'noise_psd',
                                        'presence', 'stream']
    assert protos['nele_ns_init'][3] == ['state', 'state_bytes', 'max_streams', 'stream']
    assert protos['nele_ns_reset'][3] == ['state', 'state_bytes', 'max_streams', 'slots', 'stream']
    assert protos['nele_ns_state_bytes'][3] == ['max_streams'] and protos['nele_ns_stream_record_bytes'][3] == []
    opening = src[:src.index('#ifndef')]
    assert all(name in opening for name in EARLIER_HEADERS)
    for earlier in EARLIER_HEADERS:
        assert not set(ENTRY_POINTS) & set(re.findall(r'\b(nele_[a-z0-9_]+)\s*\(', _header(earlier))), earlier
        assert not set(consts) & set(gen.consts(_header(earlier))), earlier


def test_both_libraries_export_every_entry_point_of_the_fifth_header():
    for name in ('libnele_hip.so', 'libnele_hip_ab.so'):
        lib = ctypes.CDLL(os.path.join(ROOT, 'nele_gan_amd', name))
        assert [s for s in ENTRY_POINTS if not hasattr(lib, s)] == [], name


def test_the_binding_has_the_headers_arity_and_constants_in_dicts_of_their_own():
    from nele_gan_amd import _abi, _abi_ext, _abi_ext2, _abi_ext3, _abi_ext4, _lib
    src = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    found = re.findall(r'^([a-z][a-z *]*?)\s*\b(nele_[A-Za-z0-9_]+)\s*\(([^)]*)\)\s*;', src, flags=re.M)      # read here, not by the generator
    assert sorted(f[1] for f in found) == sorted(ENTRY_POINTS) == sorted(_abi_ext4.FUNCS) == sorted(_lib.FUNCS4) == sorted(_lib._SIGS4)
    restypes = {'int': ctypes.c_int, 'longlong': ctypes.c_longlong}
    for ret, name, params in found:
        fn = getattr(_lib.lib, name)
        nargs = 0 if params.strip() == 'void' else params.count(',') + 1
        assert len(fn.argtypes) == nargs == len(_abi_ext4.FUNCS[name][1]) == len(_lib._SIGS4[name]), name
        assert fn.restype is restypes[ret.replace(' ', '')], name
    earlier = set(_abi.FUNCS) | set(_abi_ext.FUNCS) | set(_abi_ext2.FUNCS) | set(_abi_ext3.FUNCS)
    assert not set(_abi_ext4.FUNCS) & earlier
    assert not set(_lib.FUNCS4) & (set(_lib.FUNCS) | set(_lib.FUNCS2) | set(_lib.FUNCS3))
    assert not set(_lib._SIGS4) & (set(_lib._SIGS) | set(_lib._SIGS3))
    assert _abi_ext4.CONSTS == _gen_abi().consts(_header()) == _lib.CONSTS4
    assert not set(_lib.CONSTS4) & (set(_lib.CONSTS) | set(_lib.CONSTS2) | set(_lib.CONSTS3))
    # every size the four earlier ABI tests count is what it was
    assert len(_lib.FUNCS) == len(_abi.FUNCS) + len(_abi_ext.FUNCS) and len(_lib.CONSTS) == len(_abi.CONSTS) + len(_abi_ext.CONSTS)
    assert len(_lib.FUNCS2) == len(_abi_ext2.FUNCS) == 8 and len(_lib._SIGS) == len(_lib.FUNCS) + 8
    assert len(_lib.FUNCS3) == len(_abi_ext3.FUNCS) == len(_lib._SIGS3) == 7
    for name in ENTRY_POINTS:                                                    # not plan operations: the operation ids do not move
        assert _lib.lib.nele_plan_op_id(name.encode()) == -1


def _copy(tmp_path, rels):
    for rel in rels:
        os.makedirs(os.path.dirname(str(tmp_path / rel)), exist_ok=True)
        shutil.copy(os.path.join(ROOT, rel), str(tmp_path / rel))
    return str(tmp_path / 'tools' / 'gen_abi.py')


def test_check_mode_notices_a_stale_fifth_file(tmp_path):
    tool = _copy(tmp_path, ('tools/gen_abi.py',) + tuple('include/' + h for h in EARLIER_HEADERS) + ('include/nele_hip_ext4.h',) + EARLIER + (FIFTH,))
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 0
    with open(str(tmp_path / FIFTH), 'a') as f:
        f.write('# stale\n')
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 1
    assert subprocess.run([sys.executable, tool], stdout=subprocess.DEVNULL).returncode == 0
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 0
    for rel in EARLIER + (FIFTH,):
        assert open(str(tmp_path / rel)).read() == open(os.path.join(ROOT, rel)).read(), rel
    os.remove(str(tmp_path / FIFTH))                                             # a missing file is a stale one
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 1
    assert subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_abi.py'), '--check']).returncode == 0       # the tree itself


def test_a_tree_without_the_fifth_header_is_written_and_checked_as_before(tmp_path):
    tool = _copy(tmp_path, ('tools/gen_abi.py',) + tuple('include/' + h for h in EARLIER_HEADERS) + EARLIER)
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 0
    assert subprocess.run([sys.executable, tool], stdout=subprocess.DEVNULL).returncode == 0
    assert not os.path.exists(str(tmp_path / FIFTH))
    for rel in EARLIER:
        assert open(str(tmp_path / rel)).read() == open(os.path.join(ROOT, rel)).read(), rel


# ------------------------------------------------------------------------------------------------------- the entry points, no GPU
def _lib():
    from nele_gan_amd import _lib
    return _lib.lib


def test_state_bytes_are_a_header_plus_one_record_per_stream():
    lib = _lib()
    rec = lib.nele_ns_stream_record_bytes()
    # x_prev (float32), ola (float64), ten float64 and one float32 per bin of IMCRA state, two eight-slot minima rings
    assert rec >= 256 * 4 + 256 * 8 + 257 * (10 * 8 + 4) + 2 * 8 * 257 * 8 and rec % 256 == 0 and rec < 65536
    header = lib.nele_ns_state_bytes(1) - rec
    assert 0 < header <= 4096
    for B in (1, 2, 16, 1024, 4096, 1 << 20):
        assert lib.nele_ns_state_bytes(B) == header + B * rec
    for B in (0, -1, (1 << 20) + 1):
        assert lib.nele_ns_state_bytes(B) == -1


def test_bad_arguments_are_rejected_without_a_gpu():
    lib = _lib()
    B = 4
    need = lib.nele_ns_state_bytes(B)
    fake = ctypes.c_void_p(1 << 20)                                 # never dereferenced: every call below fails its checks first
    odd = ctypes.c_void_p((1 << 20) + 16)
    nan = float('nan')

    def hop(state=fake, nbytes=need, S=B, x=fake, nh=1, gmin=0.1, out=fake):
        return lib.nele_ns_hop(state, LL(nbytes), S, x, None, nh, gmin, out, None, None, None, None)

    cases = [
        (lambda: hop(state=None), b'nele_ns_hop', b'state'),
        (lambda: hop(nbytes=need - 1), b'nele_ns_hop', b'nele_ns_state_bytes'),
        (lambda: hop(S=0), b'nele_ns_hop', b'max_streams'),
        (lambda: hop(S=(1 << 20) + 1, nbytes=1 << 40), b'nele_ns_hop', b'max_streams'),
        (lambda: hop(state=odd), b'nele_ns_hop', b'256-byte aligned'),
        (lambda: hop(x=None), b'nele_ns_hop', b'null x'),
        (lambda: hop(out=None), b'nele_ns_hop', b'out'),
        (lambda: hop(nh=0), b'nele_ns_hop', b'nh'),
        (lambda: hop(nh=(1 << 20) + 1), b'nele_ns_hop', b'nh'),
        (lambda: hop(gmin=0.0), b'nele_ns_hop', b'gmin'),
        (lambda: hop(gmin=-0.1), b'nele_ns_hop', b'gmin'),
        (lambda: hop(gmin=1.5), b'nele_ns_hop', b'gmin'),
        (lambda: hop(gmin=nan), b'nele_ns_hop', b'gmin'),
        (lambda: lib.nele_ns_init(None, LL(need), B, None), b'nele_ns_init', b'state'),
        (lambda: lib.nele_ns_init(fake, LL(need - 1), B, None), b'nele_ns_init', b'nele_ns_state_bytes'),
        (lambda: lib.nele_ns_init(fake, LL(need), 0, None), b'nele_ns_init', b'max_streams'),
        (lambda: lib.nele_ns_init(odd, LL(need), B, None), b'nele_ns_init', b'256-byte aligned'),
        (lambda: lib.nele_ns_reset(None, LL(need), B, None, None), b'nele_ns_reset', b'state'),
        (lambda: lib.nele_ns_reset(fake, LL(need - 1), B, None, None), b'nele_ns_reset', b'nele_ns_state_bytes'),
        (lambda: lib.nele_ns_reset(fake, LL(need), -3, None, None), b'nele_ns_reset', b'max_streams'),
        (lambda: lib.nele_ns_reset(odd, LL(need), B, None, None), b'nele_ns_reset', b'256-byte aligned'),
    ]
    for i, (fn, name, what) in enumerate(cases):
        assert fn() == -1, (i, name, what)
        msg = lib.nele_last_error_string()
        assert name in msg and what in msg, (i, msg)


def test_python_classes_reject_bad_settings_before_touching_a_device():
    from nele_gan_amd.ns import DuplexEnhancer, NoiseSuppressor
    for kw, what in (({'streams': 0}, 'streams'), ({'gmin': 0.0}, 'gmin'), ({'gmin': 1.01}, 'gmin'), ({'gmin': float('nan')}, 'gmin')):
        with pytest.raises(ValueError, match=what):
            NoiseSuppressor(**dict({'streams': 2}, **kw))

    class Stub:
        def __init__(self, S):
            self.S = S
    with pytest.raises(ValueError, match='the suppressor 3'):
        DuplexEnhancer(Stub(2), Stub(3))
