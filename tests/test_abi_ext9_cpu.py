"""CPU: the tenth header include/nele_hip_ext9.h as a whole - it declares exactly the five entry points of the look-ahead limiter and
none of an earlier header's, both libraries export them, nele_gan_amd/_lib.py binds them with the header's arity and constants in dicts
of their own (the earlier headers' dicts and _SIGS keep their sizes), and tools/gen_abi.py --check notices a stale _abi_ext9.py - and,
in a tree without the tenth header, writes and checks what it did before.  Then the entry points themselves without a GPU: bad
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
ENTRY_POINTS = ('nele_lim_state_bytes', 'nele_lim_stream_record_bytes', 'nele_lim_init', 'nele_lim_reset', 'nele_lim_hop')
EARLIER_HEADERS = ('nele_hip.h', 'nele_hip_ext.h', 'nele_hip_ext2.h', 'nele_hip_ext3.h', 'nele_hip_ext4.h', 'nele_hip_ext5.h', 'nele_hip_ext6.h',
                   'nele_hip_ext7.h', 'nele_hip_ext8.h')
EARLIER = ('nele_gan_amd/_abi.py', 'nele_gan_amd/_abi_ext.py', 'nele_gan_amd/_abi_ext2.py', 'nele_gan_amd/_abi_ext3.py',
           'nele_gan_amd/_abi_ext4.py', 'nele_gan_amd/_abi_ext5.py', 'nele_gan_amd/_abi_ext6.py', 'nele_gan_amd/_abi_ext7.py',
           'nele_gan_amd/_abi_ext8.py', 'nele_gan_amd/csrc/plan_ops.inc')
TENTH = 'nele_gan_amd/_abi_ext9.py'


def _gen_abi():
    spec = importlib.util.spec_from_file_location('gen_abi', os.path.join(ROOT, 'tools', 'gen_abi.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _header(name='nele_hip_ext9.h'):
    return open(os.path.join(ROOT, 'include', name)).read()


def test_the_tenth_header_declares_the_five_entry_points_and_none_of_an_earlier_header():
    gen = _gen_abi()
    src = _header()
    protos = {p[0]: p for p in gen.prototypes(src)}                              # (raises unless every nele_* name is read as one prototype)
    assert sorted(protos) == sorted(ENTRY_POINTS) and len(set(ENTRY_POINTS)) == 5
    consts = gen.consts(src)
    assert consts == {'NELE_LIM_HOP': 256, 'NELE_LIM_MAX_LOOKAHEAD': 192, 'NELE_LIM_TAPS': 36}
    assert protos['nele_lim_state_bytes'][3] == ['max_streams', 'lookahead'] and protos['nele_lim_stream_record_bytes'][3] == ['lookahead']
    geometry = ['state', 'state_bytes', 'max_streams']
    assert protos['nele_lim_init'][3] == geometry + ['lookahead', 'stream'] and protos['nele_lim_reset'][3] == geometry + ['lookahead', 'slots', 'stream']
    assert protos['nele_lim_hop'][3] == geometry + ['x', 'active', 'nh', 'ceiling', 'drive', 'lookahead', 'rel', 'taps_host', 'out', 'gain', 'peak', 'stream']
    assert protos['nele_lim_hop'][2][6:11] == ['double', 'double', 'int', 'double', 'const double*']
    # the compressor's hop (the seventh header) has the same frame: state, x, active, nh in front, out and two optional outputs behind
    drc = {p[0]: p for p in gen.prototypes(_header('nele_hip_ext6.h'))}['nele_drc_hop']
    ours = protos['nele_lim_hop']
    assert ours[1] == drc[1] and ours[2][:6] == drc[2][:6] and ours[2][-5:] == drc[2][-5:] and ours[3][:6] == drc[3][:6]
    opening = src[:src.index('#ifndef')]
    assert all(name in opening for name in EARLIER_HEADERS)
    for earlier in EARLIER_HEADERS:
        assert not set(ENTRY_POINTS) & set(re.findall(r'\b(nele_[a-z0-9_]+)\s*\(', _header(earlier))), earlier
        assert not set(consts) & set(gen.consts(_header(earlier))), earlier


def test_both_libraries_export_every_entry_point_of_the_tenth_header():
    for name in ('libnele_hip.so', 'libnele_hip_ab.so'):
        lib = ctypes.CDLL(os.path.join(ROOT, 'nele_gan_amd', name))
        assert [s for s in ENTRY_POINTS if not hasattr(lib, s)] == [], name


def test_the_binding_has_the_headers_arity_and_constants_in_dicts_of_their_own():
    from nele_gan_amd import _abi, _abi_ext, _abi_ext2, _abi_ext3, _abi_ext4, _abi_ext5, _abi_ext6, _abi_ext7, _abi_ext8, _abi_ext9, _lib
    src = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    found = re.findall(r'^([a-z][a-z *]*?)\s*\b(nele_[A-Za-z0-9_]+)\s*\(([^)]*)\)\s*;', src, flags=re.M)      # read here, not by the generator
    assert sorted(f[1] for f in found) == sorted(ENTRY_POINTS) == sorted(_abi_ext9.FUNCS) == sorted(_lib.FUNCS9) == sorted(_lib._SIGS9)
    for ret, name, params in found:
        fn = getattr(_lib.lib, name)
        nargs = 0 if params.strip() == 'void' else params.count(',') + 1
        assert len(fn.argtypes) == nargs == len(_abi_ext9.FUNCS[name][1]) == len(_lib._SIGS9[name]), name
        want = ctypes.c_longlong if name.endswith('_bytes') else ctypes.c_int
        assert ret.strip() == ('long long' if name.endswith('_bytes') else 'int') and fn.restype is want, name
    assert _lib._SIGS9['nele_lim_hop'][6:10] == [ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_double]
    earlier = set(_abi.FUNCS) | set(_abi_ext.FUNCS) | set(_abi_ext2.FUNCS) | set(_abi_ext3.FUNCS) | set(_abi_ext4.FUNCS) | set(_abi_ext5.FUNCS) \
        | set(_abi_ext6.FUNCS) | set(_abi_ext7.FUNCS) | set(_abi_ext8.FUNCS)
    assert not set(_abi_ext9.FUNCS) & earlier
    before = (_lib.FUNCS, _lib.FUNCS2, _lib.FUNCS3, _lib.FUNCS4, _lib.FUNCS5, _lib.FUNCS6, _lib.FUNCS7, _lib.FUNCS8)
    assert not set(_lib.FUNCS9) & set().union(*before)
    assert not set(_lib._SIGS9) & (set(_lib._SIGS) | set(_lib._SIGS3) | set(_lib._SIGS4) | set(_lib._SIGS5) | set(_lib._SIGS6) | set(_lib._SIGS7)
                                   | set(_lib._SIGS8))
    assert _abi_ext9.CONSTS == _gen_abi().consts(_header()) == _lib.CONSTS9
    assert not set(_lib.CONSTS9) & set().union(_lib.CONSTS, _lib.CONSTS2, _lib.CONSTS3, _lib.CONSTS4, _lib.CONSTS5, _lib.CONSTS6, _lib.CONSTS7,
                                               _lib.CONSTS8)
    # every size the nine earlier ABI tests count is what it was
    assert len(_lib.FUNCS) == len(_abi.FUNCS) + len(_abi_ext.FUNCS) and len(_lib.CONSTS) == len(_abi.CONSTS) + len(_abi_ext.CONSTS)
    assert len(_lib.FUNCS2) == len(_abi_ext2.FUNCS) == 8 and len(_lib._SIGS) == len(_lib.FUNCS) + 8
    assert len(_lib.FUNCS3) == len(_abi_ext3.FUNCS) == len(_lib._SIGS3) == 7
    assert len(_lib.FUNCS4) == len(_abi_ext4.FUNCS) == len(_lib._SIGS4) == 5
    assert len(_lib.FUNCS5) == len(_abi_ext5.FUNCS) == len(_lib._SIGS5) == 3
    assert len(_lib.FUNCS6) == len(_abi_ext6.FUNCS) == len(_lib._SIGS6) == 5
    assert len(_lib.FUNCS7) == len(_abi_ext7.FUNCS) == len(_lib._SIGS7) == 5
    assert len(_lib.FUNCS8) == len(_abi_ext8.FUNCS) == len(_lib._SIGS8) == 6
    for name in ENTRY_POINTS:                                                    # not plan operations: the operation ids do not move
        assert _lib.lib.nele_plan_op_id(name.encode()) == -1


def _copy(tmp_path, rels):
    for rel in rels:
        os.makedirs(os.path.dirname(str(tmp_path / rel)), exist_ok=True)
        shutil.copy(os.path.join(ROOT, rel), str(tmp_path / rel))
    return str(tmp_path / 'tools' / 'gen_abi.py')


def test_check_mode_notices_a_stale_tenth_file(tmp_path):
    tool = _copy(tmp_path, ('tools/gen_abi.py',) + tuple('include/' + h for h in EARLIER_HEADERS) + ('include/nele_hip_ext9.h',) + EARLIER + (TENTH,))
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 0
    with open(str(tmp_path / TENTH), 'a') as f:
        f.write('# stale\n')
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 1
    res = subprocess.run([sys.executable, tool], stdout=subprocess.PIPE, universal_newlines=True)
    assert res.returncode == 0 and '_abi_ext8.py (6 entry points)' in res.stdout and '_abi_ext9.py (5 entry points)' in res.stdout
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 0
    for rel in EARLIER + (TENTH,):
        assert open(str(tmp_path / rel)).read() == open(os.path.join(ROOT, rel)).read(), rel
    os.remove(str(tmp_path / TENTH))                                             # a missing file is a stale one
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 1
    assert subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_abi.py'), '--check']).returncode == 0       # the tree itself


def test_a_tree_without_the_tenth_header_is_written_and_checked_as_before(tmp_path):
    tool = _copy(tmp_path, ('tools/gen_abi.py',) + tuple('include/' + h for h in EARLIER_HEADERS) + EARLIER)
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 0
    res = subprocess.run([sys.executable, tool], stdout=subprocess.PIPE, universal_newlines=True)
    assert res.returncode == 0 and '_abi_ext8.py (6 entry points)' in res.stdout and '_abi_ext9' not in res.stdout
    assert not os.path.exists(str(tmp_path / TENTH))
    for rel in EARLIER:
        assert open(str(tmp_path / rel)).read() == open(os.path.join(ROOT, rel)).read(), rel


# ------------------------------------------------------------------------------------------------------- the entry points, no GPU
def _lib():
    from nele_gan_amd import _lib
    return _lib.lib


def test_the_sizes_need_no_gpu():
    lib = _lib()
    al = lambda n: (n + 255) // 256 * 256
    for la in (1, 80, 111, 192):
        rec = lib.nele_lim_stream_record_bytes(la)
        assert rec == al(1184 + 8 * la) and rec % 256 == 0, la                   # counter, d, 262 float32 from byte 128, q from byte 1184
        assert lib.nele_lim_state_bytes(1, la) == 256 + rec
        assert lib.nele_lim_state_bytes(3, la) - lib.nele_lim_state_bytes(2, la) == rec
        assert lib.nele_lim_state_bytes(1 << 20, la) == 256 + (1 << 20) * rec
    assert lib.nele_lim_stream_record_bytes(80) == 2048 and lib.nele_lim_stream_record_bytes(1) == 1280 and lib.nele_lim_stream_record_bytes(192) == 2816
    assert lib.nele_lim_state_bytes(0, 80) == -1 and lib.nele_lim_state_bytes((1 << 20) + 1, 80) == -1
    for la in (0, -1, 193):
        assert lib.nele_lim_stream_record_bytes(la) == -1 and lib.nele_lim_state_bytes(4, la) == -1, la


def test_bad_arguments_are_rejected_without_a_gpu():
    lib = _lib()
    B, LA = 4, 80
    need = lib.nele_lim_state_bytes(B, LA)
    fake = ctypes.c_void_p(1 << 20)                                 # never dereferenced: every call below fails its checks first
    odd = ctypes.c_void_p((1 << 20) + 16)
    taps = (D * 36)(*([0.5] * 36))
    bad_taps = (D * 36)(*([0.5] * 35 + [float('nan')]))

    def init(state=fake, nbytes=need, S=B, la=LA):
        return lib.nele_lim_init(state, LL(nbytes), S, la, None)

    def reset(state=fake, nbytes=need, S=B, la=LA):
        return lib.nele_lim_reset(state, LL(nbytes), S, la, None, None)

    def hop(state=fake, nbytes=need, S=B, la=LA, x=fake, nh=1, c=0.89, drive=1.0, rel=0.999, f=taps, out=fake):
        return lib.nele_lim_hop(state, LL(nbytes), S, x, None, nh, c, drive, la, rel, f, out, None, None, None)

    cases = []
    for fn, name in ((init, b'nele_lim_init'), (reset, b'nele_lim_reset'), (hop, b'nele_lim_hop')):
        cases += [
            (lambda fn=fn: fn(state=None), name, b'null state'),
            (lambda fn=fn: fn(nbytes=need - 1), name, b'nele_lim_state_bytes(4, 80)'),
            (lambda fn=fn: fn(la=192), name, b'nele_lim_state_bytes(4, 192)'),            # a state laid out for another look-ahead is too small
            (lambda fn=fn: fn(S=0), name, b'max_streams'),
            (lambda fn=fn: fn(S=(1 << 20) + 1), name, b'max_streams'),
            (lambda fn=fn: fn(state=odd), name, b'256-byte aligned'),
            (lambda fn=fn: fn(la=0), name, b'lookahead=0'),
            (lambda fn=fn: fn(la=193), name, b'lookahead=193'),
        ]
    cases += [
        (lambda: hop(x=None), b'nele_lim_hop', b'null x'),
        (lambda: hop(out=None), b'nele_lim_hop', b'null x / out'),
        (lambda: hop(nh=0), b'nele_lim_hop', b'nh=0'),
        (lambda: hop(nh=(1 << 20) + 1), b'nele_lim_hop', b'nh='),
        (lambda: hop(c=0.0), b'nele_lim_hop', b'ceiling=0'),
        (lambda: hop(c=-1.0), b'nele_lim_hop', b'ceiling=-1'),
        (lambda: hop(c=float('inf')), b'nele_lim_hop', b'ceiling=inf'),
        (lambda: hop(c=float('nan')), b'nele_lim_hop', b'ceiling=nan'),
        (lambda: hop(c=1e-60), b'nele_lim_hop', b'float32'),
        (lambda: hop(drive=0.0), b'nele_lim_hop', b'drive=0'),
        (lambda: hop(drive=-2.0), b'nele_lim_hop', b'drive=-2'),
        (lambda: hop(drive=float('inf')), b'nele_lim_hop', b'drive=inf'),
        (lambda: hop(rel=1.0), b'nele_lim_hop', b'rel=1'),
        (lambda: hop(rel=-0.5), b'nele_lim_hop', b'rel=-0.5'),
        (lambda: hop(rel=float('nan')), b'nele_lim_hop', b'rel=nan'),
        (lambda: hop(f=bad_taps), b'nele_lim_hop', b'tap 35'),
    ]
    for i, (fn, name, what) in enumerate(cases):
        assert fn() == -1, (i, name, what)
        msg = lib.nele_last_error_string()
        assert name in msg and what in msg, (i, msg)


def test_the_python_class_rejects_bad_parameters_before_any_gpu_call():
    import pytest
    import limiter_ref as R
    from nele_gan_amd.limiter import StreamLimiter, db_factor, release_factor, true_peak_taps
    for kw in ({'streams': 0}, {'lookahead': 0}, {'lookahead': 193}, {'lookahead': 2.5}, {'ceiling_db': float('nan')}, {'ceiling_db': 1e6},
               {'drive_db': float('inf')}, {'drive_db': -1e6}, {'release': -1.0}, {'release': 1e30}, {'release': float('nan')}):
        with pytest.raises(ValueError):
            StreamLimiter(**dict({'streams': 2}, **kw))
    # the defaults are the contract's, bit for bit, and the taps the reference's
    assert release_factor(0.1) == R.RELEASE and release_factor(0.0) == 0.0 and db_factor(-1.0, 'ceiling_db') == R.CEILING and db_factor(0.0, 'drive_db') == 1.0
    f = true_peak_taps()
    assert f.shape == (3, 12) and f.dtype.name == 'float64' and (f == R.taps()).all() and abs(f[1].sum() - 1.0) < 2e-3 and (f[0] == f[2][::-1]).all()
