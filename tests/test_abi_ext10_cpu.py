"""CPU: the eleventh header include/nele_hip_ext10.h as a whole - it declares exactly the five entry points of the running ESTOI and
none of an earlier header's, both libraries export them, nele_gan_amd/_lib.py binds them with the header's arity and constants in dicts
of their own (the earlier headers' dicts and _SIGS keep their sizes), and tools/gen_abi.py --check notices a stale _abi_ext10.py - and,
in a tree without the eleventh header, writes and checks what it did before.  Then the entry points themselves without a GPU: bad
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
D = ctypes.c_double
ENTRY_POINTS = ('nele_mon_state_bytes', 'nele_mon_stream_record_bytes', 'nele_mon_init', 'nele_mon_reset', 'nele_mon_hop')
EARLIER_HEADERS = ('nele_hip.h', 'nele_hip_ext.h', 'nele_hip_ext2.h', 'nele_hip_ext3.h', 'nele_hip_ext4.h', 'nele_hip_ext5.h', 'nele_hip_ext6.h',
                   'nele_hip_ext7.h', 'nele_hip_ext8.h', 'nele_hip_ext9.h')
EARLIER = ('nele_gan_amd/_abi.py', 'nele_gan_amd/_abi_ext.py', 'nele_gan_amd/_abi_ext2.py', 'nele_gan_amd/_abi_ext3.py',
           'nele_gan_amd/_abi_ext4.py', 'nele_gan_amd/_abi_ext5.py', 'nele_gan_amd/_abi_ext6.py', 'nele_gan_amd/_abi_ext7.py',
           'nele_gan_amd/_abi_ext8.py', 'nele_gan_amd/_abi_ext9.py', 'nele_gan_amd/csrc/plan_ops.inc')
ELEVENTH = 'nele_gan_amd/_abi_ext10.py'
HDR = 11264                      # the geometry header and the tables behind it
REC = 22272                      # one record


def _gen_abi():
    spec = importlib.util.spec_from_file_location('gen_abi', os.path.join(ROOT, 'tools', 'gen_abi.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _header(name='nele_hip_ext10.h'):
    return open(os.path.join(ROOT, 'include', name)).read()


def test_the_eleventh_header_declares_the_five_entry_points_and_none_of_an_earlier_header():
    gen = _gen_abi()
    src = _header()
    protos = {p[0]: p for p in gen.prototypes(src)}                              # (raises unless every nele_* name is read as one prototype)
    assert sorted(protos) == sorted(ENTRY_POINTS) and len(set(ENTRY_POINTS)) == 5
    consts = gen.consts(src)
    assert consts == {'NELE_MON_HOP': 256, 'NELE_MON_STATS': 8, 'NELE_MON_MAX_LAG': 4}
    assert protos['nele_mon_state_bytes'][3] == ['max_streams'] and protos['nele_mon_stream_record_bytes'][3] == []
    geometry = ['state', 'state_bytes', 'max_streams']
    assert protos['nele_mon_init'][3] == geometry + ['lag', 'stream'] and protos['nele_mon_reset'][3] == geometry + ['slots', 'stream']
    assert protos['nele_mon_hop'][3] == geometry + ['ref', 'deg', 'add', 'active', 'nh', 'alpha', 'stats', 'seg', 'nseg', 'stream']
    assert protos['nele_mon_hop'][2][3:] == ['const float*', 'const float*', 'const float*', 'const unsigned char*', 'int', 'double', 'double*',
                                             'double*', 'int*', 'void*']
    opening = src[:src.index('#ifndef')]
    assert all(name in opening for name in EARLIER_HEADERS)
    for earlier in EARLIER_HEADERS:
        assert not set(ENTRY_POINTS) & set(re.findall(r'\b(nele_[a-z0-9_]+)\s*\(', _header(earlier))), earlier
        assert not set(consts) & set(gen.consts(_header(earlier))), earlier


def test_both_libraries_export_every_entry_point_of_the_eleventh_header():
    for name in ('libnele_hip.so', 'libnele_hip_ab.so'):
        lib = ctypes.CDLL(os.path.join(ROOT, 'nele_gan_amd', name))
        assert [s for s in ENTRY_POINTS if not hasattr(lib, s)] == [], name


def test_the_binding_has_the_headers_arity_and_constants_in_dicts_of_their_own():
    from nele_gan_amd import (_abi, _abi_ext, _abi_ext2, _abi_ext3, _abi_ext4, _abi_ext5, _abi_ext6, _abi_ext7, _abi_ext8, _abi_ext9, _abi_ext10,
                              _lib)
    src = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    found = re.findall(r'^([a-z][a-z *]*?)\s*\b(nele_[A-Za-z0-9_]+)\s*\(([^)]*)\)\s*;', src, flags=re.M)      # read here, not by the generator
    assert sorted(f[1] for f in found) == sorted(ENTRY_POINTS) == sorted(_abi_ext10.FUNCS) == sorted(_lib.FUNCS10) == sorted(_lib._SIGS10)
    for ret, name, params in found:
        fn = getattr(_lib.lib, name)
        nargs = 0 if params.strip() == 'void' else params.count(',') + 1
        assert len(fn.argtypes) == nargs == len(_abi_ext10.FUNCS[name][1]) == len(_lib._SIGS10[name]), name
        want = ctypes.c_longlong if name.endswith('_bytes') else ctypes.c_int
        assert ret.strip() == ('long long' if name.endswith('_bytes') else 'int') and fn.restype is want, name
    assert _lib._SIGS10['nele_mon_hop'][7:9] == [ctypes.c_int, ctypes.c_double]
    earlier = set(_abi.FUNCS) | set(_abi_ext.FUNCS) | set(_abi_ext2.FUNCS) | set(_abi_ext3.FUNCS) | set(_abi_ext4.FUNCS) | set(_abi_ext5.FUNCS) \
        | set(_abi_ext6.FUNCS) | set(_abi_ext7.FUNCS) | set(_abi_ext8.FUNCS) | set(_abi_ext9.FUNCS)
    assert not set(_abi_ext10.FUNCS) & earlier
    before = (_lib.FUNCS, _lib.FUNCS2, _lib.FUNCS3, _lib.FUNCS4, _lib.FUNCS5, _lib.FUNCS6, _lib.FUNCS7, _lib.FUNCS8, _lib.FUNCS9)
    assert not set(_lib.FUNCS10) & set().union(*before)
    assert not set(_lib._SIGS10) & (set(_lib._SIGS) | set(_lib._SIGS3) | set(_lib._SIGS4) | set(_lib._SIGS5) | set(_lib._SIGS6) | set(_lib._SIGS7)
                                    | set(_lib._SIGS8) | set(_lib._SIGS9))
    assert _abi_ext10.CONSTS == _gen_abi().consts(_header()) == _lib.CONSTS10
    assert not set(_lib.CONSTS10) & set().union(_lib.CONSTS, _lib.CONSTS2, _lib.CONSTS3, _lib.CONSTS4, _lib.CONSTS5, _lib.CONSTS6, _lib.CONSTS7,
                                                _lib.CONSTS8, _lib.CONSTS9)
    # every size the ten earlier ABI tests count is what it was
    assert len(_lib.FUNCS) == len(_abi.FUNCS) + len(_abi_ext.FUNCS) and len(_lib.CONSTS) == len(_abi.CONSTS) + len(_abi_ext.CONSTS)
    assert len(_lib.FUNCS2) == len(_abi_ext2.FUNCS) == 8 and len(_lib._SIGS) == len(_lib.FUNCS) + 8
    assert len(_lib.FUNCS3) == len(_abi_ext3.FUNCS) == len(_lib._SIGS3) == 7
    assert len(_lib.FUNCS4) == len(_abi_ext4.FUNCS) == len(_lib._SIGS4) == 5
    assert len(_lib.FUNCS5) == len(_abi_ext5.FUNCS) == len(_lib._SIGS5) == 3
    assert len(_lib.FUNCS6) == len(_abi_ext6.FUNCS) == len(_lib._SIGS6) == 5
    assert len(_lib.FUNCS7) == len(_abi_ext7.FUNCS) == len(_lib._SIGS7) == 5
    assert len(_lib.FUNCS8) == len(_abi_ext8.FUNCS) == len(_lib._SIGS8) == 6
    assert len(_lib.FUNCS9) == len(_abi_ext9.FUNCS) == len(_lib._SIGS9) == 5
    for name in ENTRY_POINTS:                                                    # not plan operations: the operation ids do not move
        assert _lib.lib.nele_plan_op_id(name.encode()) == -1


def _copy(tmp_path, rels):
    for rel in rels:
        os.makedirs(os.path.dirname(str(tmp_path / rel)), exist_ok=True)
        shutil.copy(os.path.join(ROOT, rel), str(tmp_path / rel))
    return str(tmp_path / 'tools' / 'gen_abi.py')


def test_check_mode_notices_a_stale_eleventh_file(tmp_path):
    tool = _copy(tmp_path, ('tools/gen_abi.py',) + tuple('include/' + h for h in EARLIER_HEADERS) + ('include/nele_hip_ext10.h',) + EARLIER + (ELEVENTH,))
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 0
    with open(str(tmp_path / ELEVENTH), 'a') as f:
        f.write('# stale\n')
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 1
    res = subprocess.run([sys.executable, tool], stdout=subprocess.PIPE, universal_newlines=True)
    assert res.returncode == 0 and '_abi_ext9.py (5 entry points)' in res.stdout and '_abi_ext10.py (5 entry points)' in res.stdout
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 0
    for rel in EARLIER + (ELEVENTH,):
        assert open(str(tmp_path / rel)).read() == open(os.path.join(ROOT, rel)).read(), rel
    os.remove(str(tmp_path / ELEVENTH))                                          # a missing file is a stale one
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 1
    assert subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_abi.py'), '--check']).returncode == 0       # the tree itself


def test_a_tree_without_the_eleventh_header_is_written_and_checked_as_before(tmp_path):
    tool = _copy(tmp_path, ('tools/gen_abi.py',) + tuple('include/' + h for h in EARLIER_HEADERS) + EARLIER)
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 0
    res = subprocess.run([sys.executable, tool], stdout=subprocess.PIPE, universal_newlines=True)
    assert res.returncode == 0 and '_abi_ext9.py (5 entry points)' in res.stdout and '_abi_ext10' not in res.stdout
    assert not os.path.exists(str(tmp_path / ELEVENTH))
    for rel in EARLIER:
        assert open(str(tmp_path / rel)).read() == open(os.path.join(ROOT, rel)).read(), rel


# ------------------------------------------------------------------------------------------------------- the entry points, no GPU
def _lib():
    from nele_gan_amd import _lib
    return _lib.lib


def test_the_sizes_need_no_gpu_and_the_record_is_the_headers():
    lib = _lib()
    rec = lib.nele_mon_stream_record_bytes()
    # the layout the header's comment documents: counters, readings, 16 kHz history, carried 10 kHz samples, the two overlap halves, the
    # ring of 30 places of 16 doubles, four hops of ref
    offsets = {'ctl': 0, 'stats': 64, 'hist': 256, 'tail': 2304, 'first': 6400, 'second': 8448, 'ring': 10496, 'ref': 18176}
    assert offsets['tail'] == offsets['hist'] + 8 * 2 * 128 and offsets['first'] == offsets['tail'] + 8 * 2 * 256
    assert offsets['second'] == offsets['first'] + 8 * 2 * 128 and offsets['ring'] == offsets['second'] + 8 * 2 * 128
    assert offsets['ref'] == offsets['ring'] + 8 * 2 * 30 * 16 and rec == offsets['ref'] + 4 * 4 * 256 == REC and rec % 256 == 0
    assert HDR == 256 + (8 * 5 * 120 + 255) // 256 * 256 + 8 * 256 + 16 * 256 and HDR % 256 == 0
    text = _header()
    for word in ('byte %d ' % v for v in offsets.values()):
        assert word in text, word
    assert '%d bytes per slot' % REC in text and 'from byte %d one record' % HDR in text and 'byte 5120' in text and 'byte 7168' in text
    assert lib.nele_mon_state_bytes(1) == HDR + rec
    assert lib.nele_mon_state_bytes(3) - lib.nele_mon_state_bytes(2) == rec
    assert lib.nele_mon_state_bytes(1 << 20) == HDR + (1 << 20) * rec
    assert lib.nele_mon_state_bytes(0) == -1 and lib.nele_mon_state_bytes(-3) == -1 and lib.nele_mon_state_bytes((1 << 20) + 1) == -1


def test_bad_arguments_are_rejected_without_a_gpu():
    lib = _lib()
    B = 4
    need = lib.nele_mon_state_bytes(B)
    fake = ctypes.c_void_p(1 << 20)                                 # never dereferenced: every call below fails its checks first
    odd = ctypes.c_void_p((1 << 20) + 16)

    def init(state=fake, nbytes=need, S=B, lag=1):
        return lib.nele_mon_init(state, LL(nbytes), S, lag, None)

    def reset(state=fake, nbytes=need, S=B):
        return lib.nele_mon_reset(state, LL(nbytes), S, None, None)

    def hop(state=fake, nbytes=need, S=B, ref=fake, nh=1, alpha=0.05):
        return lib.nele_mon_hop(state, LL(nbytes), S, ref, None, None, None, nh, D(alpha), None, None, None, None)

    cases = []
    for fn, name in ((init, b'nele_mon_init'), (reset, b'nele_mon_reset'), (hop, b'nele_mon_hop')):
        cases += [
            (lambda fn=fn: fn(state=None), name, b'null state'),
            (lambda fn=fn: fn(nbytes=need - 1), name, b'nele_mon_state_bytes(4)'),
            (lambda fn=fn: fn(S=0), name, b'max_streams'),
            (lambda fn=fn: fn(S=(1 << 20) + 1), name, b'max_streams'),
            (lambda fn=fn: fn(S=5), name, b'nele_mon_state_bytes(5)'),            # a state laid out for fewer streams is too small
            (lambda fn=fn: fn(state=odd), name, b'256-byte aligned'),
        ]
    cases += [
        (lambda: init(lag=-1), b'nele_mon_init', b'lag=-1'),
        (lambda: init(lag=5), b'nele_mon_init', b'lag=5'),
        (lambda: hop(ref=None), b'nele_mon_hop', b'null ref'),
        (lambda: hop(nh=0), b'nele_mon_hop', b'nh=0'),
        (lambda: hop(nh=(1 << 20) + 1), b'nele_mon_hop', b'nh='),
        (lambda: hop(alpha=0.0), b'nele_mon_hop', b'alpha=0'),
        (lambda: hop(alpha=1.5), b'nele_mon_hop', b'alpha=1.5'),
        (lambda: hop(alpha=-0.1), b'nele_mon_hop', b'alpha=-0.1'),
        (lambda: hop(alpha=float('nan')), b'nele_mon_hop', b'alpha=nan'),
    ]
    for i, (fn, name, what) in enumerate(cases):
        assert fn() == -1, (i, name, what)
        msg = lib.nele_last_error_string()
        assert name in msg and what in msg, (i, msg)
