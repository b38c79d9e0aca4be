"""CPU: the eighth header include/nele_hip_ext7.h as a whole - it declares exactly the five entry points of the high-band up-converter
and none of an earlier header's, both libraries export them, nele_gan_amd/_lib.py binds them with the header's arity and constants in
dicts of their own (the earlier headers' dicts and _SIGS keep their sizes), and tools/gen_abi.py --check notices a stale _abi_ext7.py -
and, in a tree without the eighth header, writes and checks what it did before.  Then the entry points themselves without a GPU: bad
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
ENTRY_POINTS = ('nele_hbup_record_bytes', 'nele_hbup_state_bytes', 'nele_hbup_init', 'nele_hbup_reset', 'nele_hbup_hop')
EARLIER_HEADERS = ('nele_hip.h', 'nele_hip_ext.h', 'nele_hip_ext2.h', 'nele_hip_ext3.h', 'nele_hip_ext4.h', 'nele_hip_ext5.h', 'nele_hip_ext6.h')
EARLIER = ('nele_gan_amd/_abi.py', 'nele_gan_amd/_abi_ext.py', 'nele_gan_amd/_abi_ext2.py', 'nele_gan_amd/_abi_ext3.py',
           'nele_gan_amd/_abi_ext4.py', 'nele_gan_amd/_abi_ext5.py', 'nele_gan_amd/_abi_ext6.py', 'nele_gan_amd/csrc/plan_ops.inc')
EIGHTH = 'nele_gan_amd/_abi_ext7.py'
UP, DOWN, K, LAG16, LAG = 3, 1, 65, 256, 960                 # 16 -> 48 kHz 'high', lag_hops 1


def _gen_abi():
    spec = importlib.util.spec_from_file_location('gen_abi', os.path.join(ROOT, 'tools', 'gen_abi.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _header(name='nele_hip_ext7.h'):
    return open(os.path.join(ROOT, 'include', name)).read()


def test_the_eighth_header_declares_the_five_entry_points_and_none_of_an_earlier_header():
    gen = _gen_abi()
    src = _header()
    protos = {p[0]: p for p in gen.prototypes(src)}                              # (raises unless every nele_* name is read as one prototype)
    assert sorted(protos) == sorted(ENTRY_POINTS) and len(set(ENTRY_POINTS)) == 5
    consts = gen.consts(src)
    assert consts == {'NELE_HBUP_MAX_LAG16': 2048, 'NELE_HBUP_MAX_LAG': 16384}
    geometry = ['state', 'state_bytes', 'max_streams', 'up', 'down', 'K', 'lag16', 'lag_dev']
    assert protos['nele_hbup_record_bytes'][3] == ['K', 'lag16', 'lag_dev'] and protos['nele_hbup_state_bytes'][3] == ['max_streams', 'K', 'lag16', 'lag_dev']
    assert protos['nele_hbup_init'][3] == geometry + ['stream'] and protos['nele_hbup_reset'][3] == geometry + ['slots', 'stream']
    assert protos['nele_hbup_hop'][3] == geometry + ['hp_dev', 'enh', 'enh_stride', 'low', 'low_stride', 'x', 'x_stride', 'gain', 'active', 'nh', 'y',
                                                     'y_stride', 'stream']
    assert protos['nele_hbup_hop'][2][8:17] == ['const double*', 'const float*', 'long long', 'const float*', 'long long', 'const float*', 'long long',
                                                'const float*', 'const unsigned char*']
    # init and reset as the stream converter's, with the two lags behind K
    rss = {p[0]: p for p in gen.prototypes(_header('nele_hip.h'))}
    for what in ('init', 'reset'):
        ours, theirs = protos['nele_hbup_' + what], rss['nele_resample_stream_' + what]
        assert ours[1] == theirs[1] and ours[2][:6] + ours[2][8:] == theirs[2] and ours[3][:6] + ours[3][8:] == theirs[3], what
    opening = src[:src.index('#ifndef')]
    assert all(name in opening for name in EARLIER_HEADERS)
    for earlier in EARLIER_HEADERS:
        assert not set(ENTRY_POINTS) & set(re.findall(r'\b(nele_[a-z0-9_]+)\s*\(', _header(earlier))), earlier
        assert not set(consts) & set(gen.consts(_header(earlier))), earlier


def test_both_libraries_export_every_entry_point_of_the_eighth_header():
    for name in ('libnele_hip.so', 'libnele_hip_ab.so'):
        lib = ctypes.CDLL(os.path.join(ROOT, 'nele_gan_amd', name))
        assert [s for s in ENTRY_POINTS if not hasattr(lib, s)] == [], name


def test_the_binding_has_the_headers_arity_and_constants_in_dicts_of_their_own():
    from nele_gan_amd import _abi, _abi_ext, _abi_ext2, _abi_ext3, _abi_ext4, _abi_ext5, _abi_ext6, _abi_ext7, _lib
    src = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    found = re.findall(r'^([a-z][a-z *]*?)\s*\b(nele_[A-Za-z0-9_]+)\s*\(([^)]*)\)\s*;', src, flags=re.M)      # read here, not by the generator
    assert sorted(f[1] for f in found) == sorted(ENTRY_POINTS) == sorted(_abi_ext7.FUNCS) == sorted(_lib.FUNCS7) == sorted(_lib._SIGS7)
    for ret, name, params in found:
        fn = getattr(_lib.lib, name)
        nargs = 0 if params.strip() == 'void' else params.count(',') + 1
        assert len(fn.argtypes) == nargs == len(_abi_ext7.FUNCS[name][1]) == len(_lib._SIGS7[name]), name
        want = ctypes.c_longlong if name.endswith('_bytes') else ctypes.c_int
        assert ret.strip() == ('long long' if name.endswith('_bytes') else 'int') and fn.restype is want, name
    earlier = set(_abi.FUNCS) | set(_abi_ext.FUNCS) | set(_abi_ext2.FUNCS) | set(_abi_ext3.FUNCS) | set(_abi_ext4.FUNCS) | set(_abi_ext5.FUNCS) \
        | set(_abi_ext6.FUNCS)
    assert not set(_abi_ext7.FUNCS) & earlier
    assert not set(_lib.FUNCS7) & (set(_lib.FUNCS) | set(_lib.FUNCS2) | set(_lib.FUNCS3) | set(_lib.FUNCS4) | set(_lib.FUNCS5) | set(_lib.FUNCS6))
    assert not set(_lib._SIGS7) & (set(_lib._SIGS) | set(_lib._SIGS3) | set(_lib._SIGS4) | set(_lib._SIGS5) | set(_lib._SIGS6))
    assert _abi_ext7.CONSTS == _gen_abi().consts(_header()) == _lib.CONSTS7
    assert not set(_lib.CONSTS7) & (set(_lib.CONSTS) | set(_lib.CONSTS2) | set(_lib.CONSTS3) | set(_lib.CONSTS4) | set(_lib.CONSTS5) | set(_lib.CONSTS6))
    # every size the seven earlier ABI tests count is what it was
    assert len(_lib.FUNCS) == len(_abi.FUNCS) + len(_abi_ext.FUNCS) and len(_lib.CONSTS) == len(_abi.CONSTS) + len(_abi_ext.CONSTS)
    assert len(_lib.FUNCS2) == len(_abi_ext2.FUNCS) == 8 and len(_lib._SIGS) == len(_lib.FUNCS) + 8
    assert len(_lib.FUNCS3) == len(_abi_ext3.FUNCS) == len(_lib._SIGS3) == 7
    assert len(_lib.FUNCS4) == len(_abi_ext4.FUNCS) == len(_lib._SIGS4) == 5
    assert len(_lib.FUNCS5) == len(_abi_ext5.FUNCS) == len(_lib._SIGS5) == 3
    assert len(_lib.FUNCS6) == len(_abi_ext6.FUNCS) == len(_lib._SIGS6) == 5
    for name in ENTRY_POINTS:                                                    # not plan operations: the operation ids do not move
        assert _lib.lib.nele_plan_op_id(name.encode()) == -1


def _copy(tmp_path, rels):
    for rel in rels:
        os.makedirs(os.path.dirname(str(tmp_path / rel)), exist_ok=True)
        shutil.copy(os.path.join(ROOT, rel), str(tmp_path / rel))
    return str(tmp_path / 'tools' / 'gen_abi.py')


def test_check_mode_notices_a_stale_eighth_file(tmp_path):
    tool = _copy(tmp_path, ('tools/gen_abi.py',) + tuple('include/' + h for h in EARLIER_HEADERS) + ('include/nele_hip_ext7.h',) + EARLIER + (EIGHTH,))
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 0
    with open(str(tmp_path / EIGHTH), 'a') as f:
        f.write('# stale\n')
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 1
    res = subprocess.run([sys.executable, tool], stdout=subprocess.PIPE, universal_newlines=True)
    assert res.returncode == 0 and '_abi_ext6.py (5 entry points)' in res.stdout and '_abi_ext7.py (5 entry points)' in res.stdout
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 0
    for rel in EARLIER + (EIGHTH,):
        assert open(str(tmp_path / rel)).read() == open(os.path.join(ROOT, rel)).read(), rel
    os.remove(str(tmp_path / EIGHTH))                                            # a missing file is a stale one
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 1
    assert subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_abi.py'), '--check']).returncode == 0       # the tree itself


def test_a_tree_without_the_eighth_header_is_written_and_checked_as_before(tmp_path):
    tool = _copy(tmp_path, ('tools/gen_abi.py',) + tuple('include/' + h for h in EARLIER_HEADERS) + EARLIER)
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 0
    res = subprocess.run([sys.executable, tool], stdout=subprocess.PIPE, universal_newlines=True)
    assert res.returncode == 0 and '_abi_ext6.py (5 entry points)' in res.stdout and '_abi_ext7' not in res.stdout
    assert not os.path.exists(str(tmp_path / EIGHTH))
    for rel in EARLIER:
        assert open(str(tmp_path / rel)).read() == open(os.path.join(ROOT, rel)).read(), rel


# ------------------------------------------------------------------------------------------------------- the entry points, no GPU
def _lib():
    from nele_gan_amd import _lib
    return _lib.lib


def test_the_sizes_need_no_gpu():
    lib = _lib()
    al = lambda n: (n + 255) // 256 * 256
    for k, lag16, lag in ((65, 256, 960), (65, 512, 3456), (21, 256, 299), (3, 0, 0), (2048, 2048, 16384)):
        rec = lib.nele_hbup_record_bytes(k, lag16, lag)
        assert rec == al(4 * (k - 1 + lag16 + lag)) and rec % 256 == 0, (k, lag16, lag)
        assert lib.nele_hbup_state_bytes(1, k, lag16, lag) == 256 + rec
        assert lib.nele_hbup_state_bytes(3, k, lag16, lag) - lib.nele_hbup_state_bytes(2, k, lag16, lag) == rec
        assert lib.nele_hbup_state_bytes(1 << 20, k, lag16, lag) == 256 + (1 << 20) * rec
    assert lib.nele_hbup_record_bytes(K, LAG16, LAG) == 5120
    assert lib.nele_hbup_state_bytes(0, K, LAG16, LAG) == -1 and lib.nele_hbup_state_bytes((1 << 20) + 1, K, LAG16, LAG) == -1
    for k, lag16, lag in ((0, 256, 960), (2049, 256, 960), (65, -1, 960), (65, 2049, 960), (65, 256, -1), (65, 256, 16385)):
        assert lib.nele_hbup_record_bytes(k, lag16, lag) == -1 and lib.nele_hbup_state_bytes(4, k, lag16, lag) == -1, (k, lag16, lag)


def test_bad_arguments_are_rejected_without_a_gpu():
    lib = _lib()
    B = 4
    need = lib.nele_hbup_state_bytes(B, K, LAG16, LAG)
    fake = ctypes.c_void_p(1 << 20)                                 # never dereferenced: every call below fails its checks first
    odd = ctypes.c_void_p((1 << 20) + 16)

    def geo(state=fake, nbytes=need, S=B, up=UP, down=DOWN, k=K, lag16=LAG16, lag=LAG):
        return (state, LL(nbytes), S, up, down, k, lag16, lag)

    def init(**kw):
        return lib.nele_hbup_init(*geo(**kw), None)

    def reset(**kw):
        return lib.nele_hbup_reset(*geo(**kw), None, None)

    def hop(hp=fake, enh=fake, se=256, low=fake, sl=256, x=fake, sx=768, nh=1, y=fake, sy=768, **kw):
        return lib.nele_hbup_hop(*geo(**kw), hp, enh, LL(se), low, LL(sl), x, LL(sx), None, None, nh, y, LL(sy), None)

    cases = []
    for fn, name in ((init, b'nele_hbup_init'), (reset, b'nele_hbup_reset'), (hop, b'nele_hbup_hop')):
        cases += [
            (lambda fn=fn: fn(state=None), name, b'null state'),
            (lambda fn=fn: fn(nbytes=need - 1), name, b'nele_hbup_state_bytes'),
            (lambda fn=fn: fn(S=0), name, b'max_streams'),
            (lambda fn=fn: fn(S=(1 << 20) + 1), name, b'max_streams'),
            (lambda fn=fn: fn(state=odd), name, b'256-byte aligned'),
            (lambda fn=fn: fn(up=0), name, b'up=0'),
            (lambda fn=fn: fn(k=64), name, b'K=64'),
            (lambda fn=fn: fn(lag16=-1), name, b'lag16=-1'),
            (lambda fn=fn: fn(lag16=2049), name, b'lag16=2049'),
            (lambda fn=fn: fn(lag=-1), name, b'lag_dev=-1'),
            (lambda fn=fn: fn(lag=16385), name, b'lag_dev=16385'),
            (lambda fn=fn: fn(up=3, down=7, k=150), name, b'256 up % down != 0'),       # 16 / 7 x 3 kHz: a hop of 109.71 samples
            (lambda fn=fn: fn(up=441, down=160, k=65), name, b'table'),               # 44.1 kHz: a table above 16 KiB comes first
        ]
    cases += [
        (lambda: hop(hp=None), b'nele_hbup_hop', b'null table'),
        (lambda: hop(enh=None), b'nele_hbup_hop', b'null table, enh'),
        (lambda: hop(low=None), b'nele_hbup_hop', b'low'),
        (lambda: hop(x=None), b'nele_hbup_hop', b'x'),
        (lambda: hop(y=None), b'nele_hbup_hop', b'y'),
        (lambda: hop(nh=0), b'nele_hbup_hop', b'nh=0'),
        (lambda: hop(nh=(1 << 20) + 1), b'nele_hbup_hop', b'nh='),
        (lambda: hop(up=6, nh=1 << 20, se=1 << 28, sl=1 << 28, sx=6 << 28, sy=6 << 28), b'nele_hbup_hop', b'2^30'),
        (lambda: hop(se=255), b'nele_hbup_hop', b'enh_stride=255'),
        (lambda: hop(sl=255), b'nele_hbup_hop', b'low_stride=255'),
        (lambda: hop(sx=767), b'nele_hbup_hop', b'x_stride=767'),
        (lambda: hop(sy=767), b'nele_hbup_hop', b'y_stride=767'),
        (lambda: hop(nh=2, sx=1535, sy=1536, se=512, sl=512), b'nele_hbup_hop', b'x_stride=1535'),
    ]
    for i, (fn, name, what) in enumerate(cases):
        assert fn() == -1, (i, name, what)
        msg = lib.nele_last_error_string()
        assert name in msg and what in msg, (i, msg)
