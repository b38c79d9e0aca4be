"""CPU: the seventh header include/nele_hip_ext6.h as a whole - it declares exactly the five entry points of the stream compressor and
none of an earlier header's, both libraries export them, nele_gan_amd/_lib.py binds them with the header's arity and constants in dicts
of their own (the earlier headers' dicts and _SIGS keep their sizes), and tools/gen_abi.py --check notices a stale _abi_ext6.py - and,
in a tree without the seventh header, writes and checks what it did before.  Then the entry points themselves without a GPU: bad
arguments rejected with the function's name, and the sizes the *_bytes functions give."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LL = ctypes.c_longlong
ENTRY_POINTS = ('nele_drc_state_bytes', 'nele_drc_stream_record_bytes', 'nele_drc_init', 'nele_drc_reset', 'nele_drc_hop')
EARLIER_HEADERS = ('nele_hip.h', 'nele_hip_ext.h', 'nele_hip_ext2.h', 'nele_hip_ext3.h', 'nele_hip_ext4.h', 'nele_hip_ext5.h')
EARLIER = ('nele_gan_amd/_abi.py', 'nele_gan_amd/_abi_ext.py', 'nele_gan_amd/_abi_ext2.py', 'nele_gan_amd/_abi_ext3.py',
           'nele_gan_amd/_abi_ext4.py', 'nele_gan_amd/_abi_ext5.py', 'nele_gan_amd/csrc/plan_ops.inc')
SEVENTH = 'nele_gan_amd/_abi_ext6.py'


def _gen_abi():
    spec = importlib.util.spec_from_file_location('gen_abi', os.path.join(ROOT, 'tools', 'gen_abi.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _header(name='nele_hip_ext6.h'):
    return open(os.path.join(ROOT, 'include', name)).read()


def test_the_seventh_header_declares_the_five_entry_points_and_none_of_an_earlier_header():
    gen = _gen_abi()
    src = _header()
    protos = {p[0]: p for p in gen.prototypes(src)}                              # (raises unless every nele_* name is read as one prototype)
    assert sorted(protos) == sorted(ENTRY_POINTS) and len(set(ENTRY_POINTS)) == 5
    consts = gen.consts(src)
    assert consts == {'NELE_DRC_HOP': 256, 'NELE_DRC_HIST': 400, 'NELE_DRC_LOOKAHEAD': 144}
    assert protos['nele_drc_hop'][3] == ['state', 'state_bytes', 'max_streams', 'x', 'active', 'nh', 'params', 'rho', 'lam', 'equalise', 'ref_level',
                                         'out', 'gain', 'level', 'stream']
    assert protos['nele_drc_hop'][2][6:10] == ['const nele_ssdrc_params*', 'double', 'double', 'int']      # the factors, not the seconds
    # init and reset as the noise suppressor's
    ns = {p[0]: p for p in gen.prototypes(_header('nele_hip_ext4.h'))}
    for what in ('state_bytes', 'stream_record_bytes', 'init', 'reset'):
        assert protos['nele_drc_' + what][1:] == ns['nele_ns_' + what][1:], what
    opening = src[:src.index('#ifndef')]
    assert all(name in opening for name in EARLIER_HEADERS)
    for earlier in EARLIER_HEADERS:
        assert not set(ENTRY_POINTS) & set(re.findall(r'\b(nele_[a-z0-9_]+)\s*\(', _header(earlier))), earlier
        assert not set(consts) & set(gen.consts(_header(earlier))), earlier


def test_both_libraries_export_every_entry_point_of_the_seventh_header():
    for name in ('libnele_hip.so', 'libnele_hip_ab.so'):
        lib = ctypes.CDLL(os.path.join(ROOT, 'nele_gan_amd', name))
        assert [s for s in ENTRY_POINTS if not hasattr(lib, s)] == [], name


def test_the_binding_has_the_headers_arity_and_constants_in_dicts_of_their_own():
    from nele_gan_amd import _abi, _abi_ext, _abi_ext2, _abi_ext3, _abi_ext4, _abi_ext5, _abi_ext6, _lib
    src = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    found = re.findall(r'^([a-z][a-z *]*?)\s*\b(nele_[A-Za-z0-9_]+)\s*\(([^)]*)\)\s*;', src, flags=re.M)      # read here, not by the generator
    assert sorted(f[1] for f in found) == sorted(ENTRY_POINTS) == sorted(_abi_ext6.FUNCS) == sorted(_lib.FUNCS6) == sorted(_lib._SIGS6)
    for ret, name, params in found:
        fn = getattr(_lib.lib, name)
        nargs = 0 if params.strip() == 'void' else params.count(',') + 1
        assert len(fn.argtypes) == nargs == len(_abi_ext6.FUNCS[name][1]) == len(_lib._SIGS6[name]), name
        want = ctypes.c_longlong if name.endswith('_bytes') else ctypes.c_int
        assert ret.strip() == ('long long' if name.endswith('_bytes') else 'int') and fn.restype is want, name
    earlier = set(_abi.FUNCS) | set(_abi_ext.FUNCS) | set(_abi_ext2.FUNCS) | set(_abi_ext3.FUNCS) | set(_abi_ext4.FUNCS) | set(_abi_ext5.FUNCS)
    assert not set(_abi_ext6.FUNCS) & earlier
    assert not set(_lib.FUNCS6) & (set(_lib.FUNCS) | set(_lib.FUNCS2) | set(_lib.FUNCS3) | set(_lib.FUNCS4) | set(_lib.FUNCS5))
    assert not set(_lib._SIGS6) & (set(_lib._SIGS) | set(_lib._SIGS3) | set(_lib._SIGS4) | set(_lib._SIGS5))
    assert _abi_ext6.CONSTS == _gen_abi().consts(_header()) == _lib.CONSTS6
    assert not set(_lib.CONSTS6) & (set(_lib.CONSTS) | set(_lib.CONSTS2) | set(_lib.CONSTS3) | set(_lib.CONSTS4) | set(_lib.CONSTS5))
    # every size the six earlier ABI tests count is what it was
    assert len(_lib.FUNCS) == len(_abi.FUNCS) + len(_abi_ext.FUNCS) and len(_lib.CONSTS) == len(_abi.CONSTS) + len(_abi_ext.CONSTS)
    assert len(_lib.FUNCS2) == len(_abi_ext2.FUNCS) == 8 and len(_lib._SIGS) == len(_lib.FUNCS) + 8
    assert len(_lib.FUNCS3) == len(_abi_ext3.FUNCS) == len(_lib._SIGS3) == 7
    assert len(_lib.FUNCS4) == len(_abi_ext4.FUNCS) == len(_lib._SIGS4) == 5
    assert len(_lib.FUNCS5) == len(_abi_ext5.FUNCS) == len(_lib._SIGS5) == 3
    for name in ENTRY_POINTS:                                                    # not plan operations: the operation ids do not move
        assert _lib.lib.nele_plan_op_id(name.encode()) == -1


def _copy(tmp_path, rels):
    for rel in rels:
        os.makedirs(os.path.dirname(str(tmp_path / rel)), exist_ok=True)
        shutil.copy(os.path.join(ROOT, rel), str(tmp_path / rel))
    return str(tmp_path / 'tools' / 'gen_abi.py')


def test_check_mode_notices_a_stale_seventh_file(tmp_path):
    tool = _copy(tmp_path, ('tools/gen_abi.py',) + tuple('include/' + h for h in EARLIER_HEADERS) + ('include/nele_hip_ext6.h',) + EARLIER + (SEVENTH,))
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 0
    with open(str(tmp_path / SEVENTH), 'a') as f:
        f.write('# stale\n')
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 1
    assert subprocess.run([sys.executable, tool], stdout=subprocess.DEVNULL).returncode == 0
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 0
    for rel in EARLIER + (SEVENTH,):
        assert open(str(tmp_path / rel)).read() == open(os.path.join(ROOT, rel)).read(), rel
    os.remove(str(tmp_path / SEVENTH))                                           # a missing file is a stale one
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 1
    assert subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_abi.py'), '--check']).returncode == 0       # the tree itself


def test_a_tree_without_the_seventh_header_is_written_and_checked_as_before(tmp_path):
    tool = _copy(tmp_path, ('tools/gen_abi.py',) + tuple('include/' + h for h in EARLIER_HEADERS) + EARLIER)
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 0
    res = subprocess.run([sys.executable, tool], stdout=subprocess.PIPE, universal_newlines=True)
    assert res.returncode == 0 and '_abi_ext5.py (3 entry points)' in res.stdout and '_abi_ext6' not in res.stdout
    assert not os.path.exists(str(tmp_path / SEVENTH))
    for rel in EARLIER:
        assert open(str(tmp_path / rel)).read() == open(os.path.join(ROOT, rel)).read(), rel


# ------------------------------------------------------------------------------------------------------- the entry points, no GPU
def _lib():
    from nele_gan_amd import _lib
    return _lib.lib


def _params(**kw):
    from nele_gan_amd.ssdrc import SsdrcParams
    return SsdrcParams(**kw).c_struct()


def test_the_sizes_need_no_gpu():
    lib = _lib()
    rec = lib.nele_drc_stream_record_bytes()
    assert rec == 1792 and rec % 256 == 0 and rec >= 64 + 5 * 8 + 4 * 400
    assert lib.nele_drc_state_bytes(1) == 256 + rec and lib.nele_drc_state_bytes(3) - lib.nele_drc_state_bytes(2) == rec
    assert lib.nele_drc_state_bytes(0) == -1 and lib.nele_drc_state_bytes((1 << 20) + 1) == -1
    assert lib.nele_drc_state_bytes(1 << 20) == 256 + (1 << 20) * rec


def test_bad_arguments_are_rejected_without_a_gpu():
    lib = _lib()
    B = 4
    need = lib.nele_drc_state_bytes(B)
    fake = ctypes.c_void_p(1 << 20)                                 # never dereferenced: every call below fails its checks first
    odd = ctypes.c_void_p((1 << 20) + 16)
    nan = float('nan')
    good = _params()

    def hop(state=fake, nbytes=need, S=B, x=fake, nh=1, p=good, rho=0.99, lam=0.98, out=fake):
        return lib.nele_drc_hop(state, LL(nbytes), S, x, None, nh, None if p is None else ctypes.byref(p), rho, lam, 1, None, out, None, None, None)

    def bad(**kw):
        p = _params()
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(p, k)[v[0]] = v[1]
            else:
                setattr(p, k, v)
        return p

    cases = [
        (lambda: lib.nele_drc_init(None, LL(need), B, None), b'nele_drc_init', b'state'),
        (lambda: lib.nele_drc_init(fake, LL(need - 1), B, None), b'nele_drc_init', b'nele_drc_state_bytes'),
        (lambda: lib.nele_drc_init(fake, LL(need), 0, None), b'nele_drc_init', b'max_streams'),
        (lambda: lib.nele_drc_init(odd, LL(need), B, None), b'nele_drc_init', b'256-byte aligned'),
        (lambda: lib.nele_drc_reset(None, LL(need), B, None, None), b'nele_drc_reset', b'state'),
        (lambda: lib.nele_drc_reset(fake, LL(need - 1), B, None, None), b'nele_drc_reset', b'nele_drc_state_bytes'),
        (lambda: lib.nele_drc_reset(fake, LL(need), (1 << 20) + 1, None, None), b'nele_drc_reset', b'max_streams'),
        (lambda: lib.nele_drc_reset(odd, LL(need), B, None, None), b'nele_drc_reset', b'256-byte aligned'),
        (lambda: hop(state=None), b'nele_drc_hop', b'state'),
        (lambda: hop(nbytes=need - 1), b'nele_drc_hop', b'nele_drc_state_bytes'),
        (lambda: hop(S=0), b'nele_drc_hop', b'max_streams'),
        (lambda: hop(state=odd), b'nele_drc_hop', b'256-byte aligned'),
        (lambda: hop(x=None), b'nele_drc_hop', b'null x'),
        (lambda: hop(out=None), b'nele_drc_hop', b'out'),
        (lambda: hop(nh=0), b'nele_drc_hop', b'nh'),
        (lambda: hop(nh=(1 << 20) + 1), b'nele_drc_hop', b'nh'),
        (lambda: hop(p=None), b'nele_drc_hop', b'params'),
        (lambda: hop(p=bad(attack=1.0)), b'nele_drc_hop', b'attack'),
        (lambda: hop(p=bad(release=-0.5)), b'nele_drc_hop', b'release'),
        (lambda: hop(p=bad(attack=nan)), b'nele_drc_hop', b'attack'),
        (lambda: hop(p=bad(e0_ratio=0.0)), b'nele_drc_hop', b'e0_ratio'),
        (lambda: hop(p=bad(e0_ratio=nan)), b'nele_drc_hop', b'e0_ratio'),
        (lambda: hop(p=bad(n_knots=1)), b'nele_drc_hop', b'n_knots'),
        (lambda: hop(p=bad(n_knots=9)), b'nele_drc_hop', b'n_knots'),
        (lambda: hop(p=bad(knot_out_db=(1, nan))), b'nele_drc_hop', b'knot 1'),
        (lambda: hop(p=bad(knot_in_db=(2, -70.0))), b'nele_drc_hop', b'ascend'),
        (lambda: hop(rho=1.0), b'nele_drc_hop', b'rho'),
        (lambda: hop(rho=-0.1), b'nele_drc_hop', b'rho'),
        (lambda: hop(rho=nan), b'nele_drc_hop', b'rho'),
        (lambda: hop(lam=1.0), b'nele_drc_hop', b'lam'),
        (lambda: hop(lam=nan), b'nele_drc_hop', b'lam'),
    ]
    for i, (fn, name, what) in enumerate(cases):
        assert fn() == -1, (i, name, what)
        msg = lib.nele_last_error_string()
        assert name in msg and what in msg, (i, msg)
