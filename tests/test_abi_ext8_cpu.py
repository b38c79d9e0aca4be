"""CPU: the ninth header include/nele_hip_ext8.h as a whole - it declares exactly the six entry points of the scheduled high-band
up-converter and none of an earlier header's, both libraries export them, nele_gan_amd/_lib.py binds them with the header's arity and
constants in dicts of their own (the earlier headers' dicts and _SIGS keep their sizes), and tools/gen_abi.py --check notices a stale
_abi_ext8.py - and, in a tree without the ninth header, writes and checks what it did before.  Then the entry points themselves without
a GPU: the plan, bad arguments rejected with the function's name, and the sizes the *_bytes functions give."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LL = ctypes.c_longlong
ENTRY_POINTS = ('nele_hbsched_plan', 'nele_hbsched_record_bytes', 'nele_hbsched_state_bytes', 'nele_hbsched_init', 'nele_hbsched_reset',
                'nele_hbsched_hop')
INFO = ('K', 'D_UP', 'S', 'L0', 'E', 'H', 'LAM', 'LX', 'RNUM', 'P', 'HOP_MIN', 'HOP_MAX')
EARLIER_HEADERS = ('nele_hip.h', 'nele_hip_ext.h', 'nele_hip_ext2.h', 'nele_hip_ext3.h', 'nele_hip_ext4.h', 'nele_hip_ext5.h', 'nele_hip_ext6.h',
                   'nele_hip_ext7.h')
EARLIER = ('nele_gan_amd/_abi.py', 'nele_gan_amd/_abi_ext.py', 'nele_gan_amd/_abi_ext2.py', 'nele_gan_amd/_abi_ext3.py',
           'nele_gan_amd/_abi_ext4.py', 'nele_gan_amd/_abi_ext5.py', 'nele_gan_amd/_abi_ext6.py', 'nele_gan_amd/_abi_ext7.py',
           'nele_gan_amd/csrc/plan_ops.inc')
NINTH = 'nele_gan_amd/_abi_ext8.py'
UP, DOWN, ZEROS, K, H, SHIFT, LAM, LX = 441, 160, 32, 65, 65, 32, 256, 883      # 16 -> 44.1 kHz 'high', lag_hops 1, D_down 32


def _gen_abi():
    spec = importlib.util.spec_from_file_location('gen_abi', os.path.join(ROOT, 'tools', 'gen_abi.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _header(name='nele_hip_ext8.h'):
    return open(os.path.join(ROOT, 'include', name)).read()


def test_the_ninth_header_declares_the_six_entry_points_and_none_of_an_earlier_header():
    gen = _gen_abi()
    src = _header()
    protos = {p[0]: p for p in gen.prototypes(src)}                              # (raises unless every nele_* name is read as one prototype)
    assert sorted(protos) == sorted(ENTRY_POINTS) and len(set(ENTRY_POINTS)) == 6
    consts = gen.consts(src)
    assert consts == dict({'NELE_HBSCHED_INFO': 12}, **{'NELE_HBSCHED_I_' + n: i for i, n in enumerate(INFO)})
    geometry = ['state', 'state_bytes', 'max_streams', 'up', 'down', 'K', 's', 'lam', 'Lx']
    assert protos['nele_hbsched_plan'][3] == ['up', 'down', 'zeros', 'lag_hops', 'd_down', 'info_host'] and protos['nele_hbsched_plan'][2][-1] == 'int*'
    assert protos['nele_hbsched_record_bytes'][3] == ['H', 'lam', 'Lx'] and protos['nele_hbsched_state_bytes'][3] == ['max_streams', 'H', 'lam', 'Lx']
    assert protos['nele_hbsched_init'][3] == geometry + ['stream'] and protos['nele_hbsched_reset'][3] == geometry + ['slots', 'stream']
    assert protos['nele_hbsched_hop'][3] == geometry + ['hp_dev', 'enh', 'enh_stride', 'low', 'low_stride', 'x', 'x_stride', 'gain', 'active', 'nh',
                                                        'pos', 'y', 'y_stride', 'stream']
    # the hop as the unscheduled one's, with s in front of the two lags and pos behind nh
    hb = {p[0]: p for p in gen.prototypes(_header('nele_hip_ext7.h'))}['nele_hbup_hop']
    ours = protos['nele_hbsched_hop']
    assert ours[1] == hb[1] and ours[2][:6] + ours[2][7:19] + ours[2][20:] == hb[2] and ours[3][9:19] + ours[3][20:] == hb[3][8:]
    assert ours[2][6] == 'int' and ours[2][19] == 'int'
    opening = src[:src.index('#ifndef')]
    assert all(name in opening for name in EARLIER_HEADERS)
    for earlier in EARLIER_HEADERS:
        assert not set(ENTRY_POINTS) & set(re.findall(r'\b(nele_[a-z0-9_]+)\s*\(', _header(earlier))), earlier
        assert not set(consts) & set(gen.consts(_header(earlier))), earlier


def test_both_libraries_export_every_entry_point_of_the_ninth_header():
    for name in ('libnele_hip.so', 'libnele_hip_ab.so'):
        lib = ctypes.CDLL(os.path.join(ROOT, 'nele_gan_amd', name))
        assert [s for s in ENTRY_POINTS if not hasattr(lib, s)] == [], name


def test_the_binding_has_the_headers_arity_and_constants_in_dicts_of_their_own():
    from nele_gan_amd import _abi, _abi_ext, _abi_ext2, _abi_ext3, _abi_ext4, _abi_ext5, _abi_ext6, _abi_ext7, _abi_ext8, _lib
    src = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    found = re.findall(r'^([a-z][a-z *]*?)\s*\b(nele_[A-Za-z0-9_]+)\s*\(([^)]*)\)\s*;', src, flags=re.M)      # read here, not by the generator
    assert sorted(f[1] for f in found) == sorted(ENTRY_POINTS) == sorted(_abi_ext8.FUNCS) == sorted(_lib.FUNCS8) == sorted(_lib._SIGS8)
    for ret, name, params in found:
        fn = getattr(_lib.lib, name)
        nargs = 0 if params.strip() == 'void' else params.count(',') + 1
        assert len(fn.argtypes) == nargs == len(_abi_ext8.FUNCS[name][1]) == len(_lib._SIGS8[name]), name
        want = ctypes.c_longlong if name.endswith('_bytes') else ctypes.c_int
        assert ret.strip() == ('long long' if name.endswith('_bytes') else 'int') and fn.restype is want, name
    earlier = set(_abi.FUNCS) | set(_abi_ext.FUNCS) | set(_abi_ext2.FUNCS) | set(_abi_ext3.FUNCS) | set(_abi_ext4.FUNCS) | set(_abi_ext5.FUNCS) \
        | set(_abi_ext6.FUNCS) | set(_abi_ext7.FUNCS)
    assert not set(_abi_ext8.FUNCS) & earlier
    before = (_lib.FUNCS, _lib.FUNCS2, _lib.FUNCS3, _lib.FUNCS4, _lib.FUNCS5, _lib.FUNCS6, _lib.FUNCS7)
    assert not set(_lib.FUNCS8) & set().union(*before)
    assert not set(_lib._SIGS8) & (set(_lib._SIGS) | set(_lib._SIGS3) | set(_lib._SIGS4) | set(_lib._SIGS5) | set(_lib._SIGS6) | set(_lib._SIGS7))
    assert _abi_ext8.CONSTS == _gen_abi().consts(_header()) == _lib.CONSTS8
    assert not set(_lib.CONSTS8) & set().union(_lib.CONSTS, _lib.CONSTS2, _lib.CONSTS3, _lib.CONSTS4, _lib.CONSTS5, _lib.CONSTS6, _lib.CONSTS7)
    # every size the eight earlier ABI tests count is what it was
    assert len(_lib.FUNCS) == len(_abi.FUNCS) + len(_abi_ext.FUNCS) and len(_lib.CONSTS) == len(_abi.CONSTS) + len(_abi_ext.CONSTS)
    assert len(_lib.FUNCS2) == len(_abi_ext2.FUNCS) == 8 and len(_lib._SIGS) == len(_lib.FUNCS) + 8
    assert len(_lib.FUNCS3) == len(_abi_ext3.FUNCS) == len(_lib._SIGS3) == 7
    assert len(_lib.FUNCS4) == len(_abi_ext4.FUNCS) == len(_lib._SIGS4) == 5
    assert len(_lib.FUNCS5) == len(_abi_ext5.FUNCS) == len(_lib._SIGS5) == 3
    assert len(_lib.FUNCS6) == len(_abi_ext6.FUNCS) == len(_lib._SIGS6) == 5
    assert len(_lib.FUNCS7) == len(_abi_ext7.FUNCS) == len(_lib._SIGS7) == 5
    for name in ENTRY_POINTS:                                                    # not plan operations: the operation ids do not move
        assert _lib.lib.nele_plan_op_id(name.encode()) == -1


def _copy(tmp_path, rels):
    for rel in rels:
        os.makedirs(os.path.dirname(str(tmp_path / rel)), exist_ok=True)
        shutil.copy(os.path.join(ROOT, rel), str(tmp_path / rel))
    return str(tmp_path / 'tools' / 'gen_abi.py')


def test_check_mode_notices_a_stale_ninth_file(tmp_path):
    tool = _copy(tmp_path, ('tools/gen_abi.py',) + tuple('include/' + h for h in EARLIER_HEADERS) + ('include/nele_hip_ext8.h',) + EARLIER + (NINTH,))
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 0
    with open(str(tmp_path / NINTH), 'a') as f:
        f.write('# stale\n')
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 1
    res = subprocess.run([sys.executable, tool], stdout=subprocess.PIPE, universal_newlines=True)
    assert res.returncode == 0 and '_abi_ext7.py (5 entry points)' in res.stdout and '_abi_ext8.py (6 entry points)' in res.stdout
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 0
    for rel in EARLIER + (NINTH,):
        assert open(str(tmp_path / rel)).read() == open(os.path.join(ROOT, rel)).read(), rel
    os.remove(str(tmp_path / NINTH))                                             # a missing file is a stale one
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 1
    assert subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_abi.py'), '--check']).returncode == 0       # the tree itself


def test_a_tree_without_the_ninth_header_is_written_and_checked_as_before(tmp_path):
    tool = _copy(tmp_path, ('tools/gen_abi.py',) + tuple('include/' + h for h in EARLIER_HEADERS) + EARLIER)
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 0
    res = subprocess.run([sys.executable, tool], stdout=subprocess.PIPE, universal_newlines=True)
    assert res.returncode == 0 and '_abi_ext7.py (5 entry points)' in res.stdout and '_abi_ext8' not in res.stdout
    assert not os.path.exists(str(tmp_path / NINTH))
    for rel in EARLIER:
        assert open(str(tmp_path / rel)).read() == open(os.path.join(ROOT, rel)).read(), rel


# ------------------------------------------------------------------------------------------------------- the entry points, no GPU
def _lib():
    from nele_gan_amd import _lib
    return _lib.lib


def _plan(up, down, zeros, lag_hops, d_down):
    info = (ctypes.c_int * 12)()
    st = _lib().nele_hbsched_plan(up, down, zeros, lag_hops, d_down, info)
    return st, dict(zip(INFO, info))


def test_the_plan_needs_no_gpu():
    st, p = _plan(UP, DOWN, ZEROS, 1, 32)
    assert st == 0 and p == {'K': K, 'D_UP': 89, 'S': SHIFT, 'L0': -160, 'E': 1, 'H': H, 'LAM': LAM, 'LX': LX, 'RNUM': 3528, 'P': 5, 'HOP_MIN': 705,
                             'HOP_MAX': 706}
    st, p = _plan(UP, DOWN, 10, 1, 10)                               # 'scipy'
    assert st == 0 and (p['S'], p['LX'], p['L0'], p['E']) == (134, 762, -204, 1)
    st, p = _plan(441, 320, 10, 1, 10)                               # 22.05 kHz 'scipy': the shifted lead needs a second sample of history
    assert st == 0 and (p['S'], p['LX'], p['L0'], p['E'], p['H']) == (134, 381, -204, 2, p['K'] + 1)
    st, p = _plan(3, 1, ZEROS, 1, 32)                                # 48 kHz: section 24's figures
    assert st == 0 and (p['S'], p['LX'], p['L0'], p['E'], p['H'], p['P'], p['HOP_MIN'], p['HOP_MAX']) == (0, 960, 0, 0, 64, 1, 768, 768)
    lib = _lib()
    for args, what in (((0, DOWN, ZEROS, 1, 32), b'up=0'), ((UP, DOWN, 0, 1, 32), b'zeros=0'), ((UP, DOWN, 65, 1, 32), b'zeros=65'),
                       ((UP, DOWN, ZEROS, 0, 32), b'lag_hops=0'), ((UP, DOWN, ZEROS, 9, 32), b'lag_hops=9'), ((UP, DOWN, ZEROS, 1, -1), b'd_down=-1'),
                       ((UP, DOWN, ZEROS, 1, 257), b'd_down=257'), ((1, 2, ZEROS, 1, 32), b'no band'), ((1, 1, ZEROS, 1, 32), b'no band'),
                       ((160, 441, ZEROS, 1, 32), b'no band')):
        assert _plan(*args)[0] == -1, args
        msg = lib.nele_last_error_string()
        assert b'nele_hbsched_plan' in msg and what in msg, (args, msg)
    assert lib.nele_hbsched_plan(UP, DOWN, ZEROS, 1, 32, None) == -1 and b'null info_host' in lib.nele_last_error_string()


def test_the_sizes_need_no_gpu():
    lib = _lib()
    al = lambda n: (n + 255) // 256 * 256
    for h, lam, lx in ((65, 256, 883), (65, 512, 1589), (21, 256, 381), (0, 0, 0), (4096, 2048, 16384)):
        rec = lib.nele_hbsched_record_bytes(h, lam, lx)
        assert rec == al(16 + 4 * (h + lam + lx)) and rec % 256 == 0, (h, lam, lx)
        assert lib.nele_hbsched_state_bytes(1, h, lam, lx) == 256 + rec
        assert lib.nele_hbsched_state_bytes(3, h, lam, lx) - lib.nele_hbsched_state_bytes(2, h, lam, lx) == rec
        assert lib.nele_hbsched_state_bytes(1 << 20, h, lam, lx) == 256 + (1 << 20) * rec
    assert lib.nele_hbsched_record_bytes(H, LAM, LX) == 4864                     # 16 + 4 x 1204 = 4832
    assert lib.nele_hbsched_state_bytes(0, H, LAM, LX) == -1 and lib.nele_hbsched_state_bytes((1 << 20) + 1, H, LAM, LX) == -1
    for h, lam, lx in ((-1, 256, 883), (4097, 256, 883), (65, -1, 883), (65, 2049, 883), (65, 256, -1), (65, 256, 16385)):
        assert lib.nele_hbsched_record_bytes(h, lam, lx) == -1 and lib.nele_hbsched_state_bytes(4, h, lam, lx) == -1, (h, lam, lx)


def test_bad_arguments_are_rejected_without_a_gpu():
    lib = _lib()
    B = 4
    need = lib.nele_hbsched_state_bytes(B, H, LAM, LX)
    fake = ctypes.c_void_p(1 << 20)                                 # never dereferenced: every call below fails its checks first
    odd = ctypes.c_void_p((1 << 20) + 16)

    def geo(state=fake, nbytes=need, S=B, up=UP, down=DOWN, k=K, s=SHIFT, lam=LAM, lx=LX):
        return (state, LL(nbytes), S, up, down, k, s, lam, lx)

    def init(**kw):
        return lib.nele_hbsched_init(*geo(**kw), None)

    def reset(**kw):
        return lib.nele_hbsched_reset(*geo(**kw), None, None)

    def hop(hp=fake, enh=fake, se=256, low=fake, sl=256, x=fake, sx=705, nh=1, pos=0, y=fake, sy=705, **kw):
        return lib.nele_hbsched_hop(*geo(**kw), hp, enh, LL(se), low, LL(sl), x, LL(sx), None, None, nh, pos, y, LL(sy), None)

    cases = []
    for fn, name in ((init, b'nele_hbsched_init'), (reset, b'nele_hbsched_reset'), (hop, b'nele_hbsched_hop')):
        cases += [
            (lambda fn=fn: fn(state=None), name, b'null state'),
            (lambda fn=fn: fn(nbytes=need - 1), name, b'nele_hbsched_state_bytes'),
            (lambda fn=fn: fn(S=0), name, b'max_streams'),
            (lambda fn=fn: fn(S=(1 << 20) + 1), name, b'max_streams'),
            (lambda fn=fn: fn(state=odd), name, b'256-byte aligned'),
            (lambda fn=fn: fn(up=0), name, b'up=0'),
            (lambda fn=fn: fn(k=64), name, b'K=64'),
            (lambda fn=fn: fn(up=160, down=441, k=177), name, b'no band'),
            (lambda fn=fn: fn(s=-1), name, b's=-1'),
            (lambda fn=fn: fn(s=160), name, b's=160'),
            (lambda fn=fn: fn(lam=-256), name, b'lam=-256'),
            (lambda fn=fn: fn(lam=255), name, b'lam=255'),
            (lambda fn=fn: fn(lam=2304), name, b'lam=2304'),
            (lambda fn=fn: fn(lx=-1), name, b'Lx=-1'),
            (lambda fn=fn: fn(lx=16385), name, b'Lx=16385'),
            (lambda fn=fn: fn(lx=884), name, b'Lx=884 is not'),                         # no D_down gives it with this s
            (lambda fn=fn: fn(s=0), name, b'Lx=883 is not'),                            # nor this s with that Lx: the unshifted lead is refused
            (lambda fn=fn: fn(lx=88), name, b'Lx=88 is not'),                           # a negative D_down
        ]
    cases += [
        (lambda: hop(hp=None), b'nele_hbsched_hop', b'null table'),
        (lambda: hop(enh=None), b'nele_hbsched_hop', b'null table, enh'),
        (lambda: hop(low=None), b'nele_hbsched_hop', b'low'),
        (lambda: hop(x=None), b'nele_hbsched_hop', b'x'),
        (lambda: hop(y=None), b'nele_hbsched_hop', b'y'),
        (lambda: hop(nh=0), b'nele_hbsched_hop', b'nh=0'),
        (lambda: hop(nh=(1 << 20) + 1), b'nele_hbsched_hop', b'nh='),
        (lambda: hop(pos=-1), b'nele_hbsched_hop', b'pos=-1'),
        (lambda: hop(pos=5), b'nele_hbsched_hop', b'pos=5'),
        (lambda: hop(up=441, down=80, lx=1765, nbytes=1 << 33, nh=1 << 20, se=1 << 28, sl=1 << 28, sx=1 << 31, sy=1 << 31), b'nele_hbsched_hop',
         b'2^30'),                                                                       # 88.2 kHz: 2^20 hops of 1411.2 samples
        (lambda: hop(se=255), b'nele_hbsched_hop', b'enh_stride=255'),
        (lambda: hop(sl=255), b'nele_hbsched_hop', b'low_stride=255'),
        (lambda: hop(sx=704), b'nele_hbsched_hop', b'x_stride=704'),
        (lambda: hop(sy=704), b'nele_hbsched_hop', b'y_stride=704'),
        (lambda: hop(pos=1, sx=705, sy=706), b'nele_hbsched_hop', b'x_stride=705'),     # the hop at position 1 is 706 samples
        (lambda: hop(nh=2, sx=1410, sy=1411, se=512, sl=512), b'nele_hbsched_hop', b'x_stride=1410'),
    ]
    for i, (fn, name, what) in enumerate(cases):
        assert fn() == -1, (i, name, what)
        msg = lib.nele_last_error_string()
        assert name in msg and what in msg, (i, msg)
