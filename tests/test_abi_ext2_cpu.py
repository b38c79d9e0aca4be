"""CPU: the third header include/nele_hip_ext2.h as a whole - it declares exactly the eight entry points of the clock-drift compensator,
both libraries export them, nele_gan_amd/_lib.py binds them with the header's arity and constants in dicts of their own (the two
earlier headers' dicts keep their sizes), and tools/gen_abi.py --check notices a stale _abi_ext2.py - and, in a tree without the third
header, writes and checks what it always has."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('nele_drift_state_bytes', 'nele_drift_stream_record_bytes', 'nele_drift_init', 'nele_drift_reset', 'nele_drift_set_rate',
                'nele_drift_hop', 'nele_drift_status', 'nele_drift_taps')
CONSTS = {'NELE_DRIFT_PHASES': 64, 'NELE_DRIFT_TAPS': 64, 'NELE_DRIFT_BETA': 8.0, 'NELE_DRIFT_SMOOTH': 0.9, 'NELE_DRIFT_EPS': 1e-6,
          'NELE_DRIFT_TINY': 1e-12, 'NELE_DRIFT_WARM': 32, 'NELE_DRIFT_MAX_RATE': 1e-3, 'NELE_DRIFT_INFO': 6}
EARLIER = ('nele_gan_amd/_abi.py', 'nele_gan_amd/_abi_ext.py', 'nele_gan_amd/csrc/plan_ops.inc')
THIRD = 'nele_gan_amd/_abi_ext2.py'


def _gen_abi():
    spec = importlib.util.spec_from_file_location('gen_abi', os.path.join(ROOT, 'tools', 'gen_abi.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _header(name='nele_hip_ext2.h'):
    return open(os.path.join(ROOT, 'include', name)).read()


def test_the_third_header_declares_the_eight_entry_points_and_says_what_it_is_for():
    gen = _gen_abi()
    src = _header()
    protos = {p[0]: p for p in gen.prototypes(src)}                              # (raises unless every nele_* name is read as one prototype)
    assert sorted(protos) == sorted(ENTRY_POINTS) and len(set(ENTRY_POINTS)) == 8
    consts = gen.consts(src)
    assert {k: consts[k] for k in CONSTS} == CONSTS
    assert sorted(v for k, v in consts.items() if k.startswith('NELE_DRIFT_I_')) == list(range(6)) and len(consts) == len(CONSTS) + 6
    assert protos['nele_drift_hop'][3] == ['state', 'state_bytes', 'max_streams', 'blocks', 'mic', 'played', 'base_hops', 'active', 'adapt', 'nh',
                                           'lam_fast', 'lam_slow', 'kp', 'ki', 'aligned', 'snapped', 'stream']
    assert protos['nele_drift_set_rate'][3] == ['state', 'state_bytes', 'max_streams', 'blocks', 'slots', 'rate_dev', 'stream']
    assert protos['nele_drift_taps'][3] == ['state', 'state_bytes', 'max_streams', 'blocks', 'taps_out_dev', 'stream']
    opening = src[:src.index('#ifndef')]
    assert 'nele_hip.h' in opening and 'nele_hip_ext.h' in opening and '19' in opening
    for earlier in ('nele_hip.h', 'nele_hip_ext.h'):
        assert not set(ENTRY_POINTS) & set(re.findall(r'\b(nele_[a-z0-9_]+)\s*\(', _header(earlier))), earlier


def test_both_libraries_export_every_entry_point_of_the_third_header():
    for name in ('libnele_hip.so', 'libnele_hip_ab.so'):
        lib = ctypes.CDLL(os.path.join(ROOT, 'nele_gan_amd', name))
        assert [s for s in ENTRY_POINTS if not hasattr(lib, s)] == [], name


def test_the_binding_has_the_headers_arity_and_constants_in_dicts_of_their_own():
    from nele_gan_amd import _abi, _abi_ext, _abi_ext2, _lib
    src = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    found = re.findall(r'^([a-z][a-z *]*?)\s*\b(nele_[A-Za-z0-9_]+)\s*\(([^)]*)\)\s*;', src, flags=re.M)      # read here, not by the generator
    assert sorted(f[1] for f in found) == sorted(ENTRY_POINTS) == sorted(_abi_ext2.FUNCS) == sorted(_lib.FUNCS2)
    restypes = {'int': ctypes.c_int, 'longlong': ctypes.c_longlong}
    for ret, name, params in found:
        fn = getattr(_lib.lib, name)
        nargs = 0 if params.strip() == 'void' else params.count(',') + 1
        assert len(fn.argtypes) == nargs == len(_abi_ext2.FUNCS[name][1]) == len(_lib._SIGS[name]), name
        assert fn.restype is restypes[ret.replace(' ', '')], name
    assert not set(_abi_ext2.FUNCS) & (set(_abi.FUNCS) | set(_abi_ext.FUNCS)) and not set(_lib.FUNCS2) & set(_lib.FUNCS)
    assert _abi_ext2.CONSTS == _gen_abi().consts(_header()) == _lib.CONSTS2 and not set(_lib.CONSTS2) & set(_lib.CONSTS)
    assert len(_lib.FUNCS) == len(_abi.FUNCS) + len(_abi_ext.FUNCS) and len(_lib.CONSTS) == len(_abi.CONSTS) + len(_abi_ext.CONSTS)
    assert len(_lib._SIGS) == len(_lib.FUNCS) + 8
    for name in ENTRY_POINTS:                                                    # not plan operations: the operation ids do not move
        assert _lib.lib.nele_plan_op_id(name.encode()) == -1


def _copy(tmp_path, rels):
    for rel in rels:
        os.makedirs(os.path.dirname(str(tmp_path / rel)), exist_ok=True)
        shutil.copy(os.path.join(ROOT, rel), str(tmp_path / rel))
    return str(tmp_path / 'tools' / 'gen_abi.py')


def test_check_mode_notices_a_stale_third_file(tmp_path):
    tool = _copy(tmp_path, ('tools/gen_abi.py', 'include/nele_hip.h', 'include/nele_hip_ext.h', 'include/nele_hip_ext2.h') + EARLIER + (THIRD,))
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 0
    with open(str(tmp_path / THIRD), 'a') as f:
        f.write('# stale\n')
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 1
    assert subprocess.run([sys.executable, tool], stdout=subprocess.DEVNULL).returncode == 0
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 0
    for rel in EARLIER + (THIRD,):
        assert open(str(tmp_path / rel)).read() == open(os.path.join(ROOT, rel)).read(), rel
    os.remove(str(tmp_path / THIRD))                                             # a missing file is a stale one
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 1
    assert subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_abi.py'), '--check']).returncode == 0       # the tree itself


def test_a_tree_without_the_third_header_is_written_and_checked_as_before(tmp_path):
    tool = _copy(tmp_path, ('tools/gen_abi.py', 'include/nele_hip.h', 'include/nele_hip_ext.h') + EARLIER)
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 0
    assert subprocess.run([sys.executable, tool], stdout=subprocess.DEVNULL).returncode == 0
    assert not os.path.exists(str(tmp_path / THIRD))
    for rel in EARLIER:
        assert open(str(tmp_path / rel)).read() == open(os.path.join(ROOT, rel)).read(), rel
