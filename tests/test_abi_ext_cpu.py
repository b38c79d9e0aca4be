"""CPU: the extension header include/nele_hip_ext.h as a whole - it declares exactly the entry points of the three features that live
in it (the bulk-delay search, the delay tracker, the residual-echo suppressor: each feature's own CPU test holds its list), both
libraries export them, nele_gan_amd/_lib.py binds them with the header's arity and constants, and tools/gen_abi.py --check notices each
generated file going stale."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess
import sys

from tests.test_bulk_cpu import ENTRY_POINTS as BULK
from tests.test_res_cpu import ENTRY_POINTS as RES
from tests.test_track_cpu import ENTRY_POINTS as TRACK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = BULK + TRACK + RES
GENERATED = ('nele_gan_amd/_abi.py', 'nele_gan_amd/_abi_ext.py', 'nele_gan_amd/csrc/plan_ops.inc')


def _gen_abi():
    spec = importlib.util.spec_from_file_location('gen_abi', os.path.join(ROOT, 'tools', 'gen_abi.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _ext_header():
    return open(os.path.join(ROOT, 'include', 'nele_hip_ext.h')).read()


def test_the_extension_header_declares_the_three_features_and_says_what_it_is_for():
    gen = _gen_abi()
    src = _ext_header()
    assert (len(BULK), len(RES), len(TRACK)) == (7, 5, 7) and len(set(ENTRY_POINTS)) == 19
    protos = {p[0]: p for p in gen.prototypes(src)}                              # (raises unless every nele_* name is read as one prototype)
    assert sorted(protos) == sorted(ENTRY_POINTS)
    consts = gen.consts(src)
    assert {k: v for k, v in consts.items() if k.startswith('NELE_BULK_')} == {'NELE_BULK_MAX_BLOCKS': 64, 'NELE_BULK_SMOOTH': 0.9, 'NELE_BULK_EPS': 1e-6}
    assert {k: v for k, v in consts.items() if k.startswith('NELE_RES_')} == {'NELE_RES_SMOOTH': 0.9, 'NELE_RES_EPS': 1e-10}
    assert consts['NELE_TRACK_INFO'] == 8 and sorted(v for k, v in consts.items() if k.startswith('NELE_TRACK_I_')) == list(range(8))
    assert protos['nele_bulk_hop'][3] == ['state', 'state_bytes', 'max_streams', 'blocks', 'mic', 'played', 'active', 'nh', 'lambda', 'ratio', 'hold',
                                          'aligned', 'delay_hops', 'stream']
    assert protos['nele_res_hop'][3] == ['state', 'state_bytes', 'max_streams', 'residual', 'echo', 'active', 'nh', 'beta', 'gmin', 'out', 'gains',
                                         'stream']
    assert protos['nele_track_hop'][3] == ['state', 'state_bytes', 'max_streams', 'blocks', 'mic', 'played', 'active', 'nh', 'lambda', 'ratio',
                                           'hold', 'patience', 'rest', 'aligned', 'moved', 'stream']
    opening = src[:src.index('#ifndef')]
    assert 'nele_hip.h' in opening and '198' in opening                          # the opening comment: entry points added after the 198
    first = open(os.path.join(ROOT, 'include', 'nele_hip.h')).read()
    assert not set(ENTRY_POINTS) & set(re.findall(r'\b(nele_[a-z0-9_]+)\s*\(', first))


def test_both_libraries_export_every_entry_point_of_the_extension_header():
    for name in ('libnele_hip.so', 'libnele_hip_ab.so'):
        lib = ctypes.CDLL(os.path.join(ROOT, 'nele_gan_amd', name))
        assert [s for s in ENTRY_POINTS if not hasattr(lib, s)] == [], name


def test_the_binding_has_the_headers_arity_and_constants_and_the_generated_files_are_current():
    from nele_gan_amd import _abi, _abi_ext, _lib
    src = re.sub(r'/\*.*?\*/', '', _ext_header(), flags=re.S)
    found = re.findall(r'^([a-z][a-z *]*?)\s*\b(nele_[A-Za-z0-9_]+)\s*\(([^)]*)\)\s*;', src, flags=re.M)      # read here, not by the generator
    assert sorted(f[1] for f in found) == sorted(ENTRY_POINTS) == sorted(_abi_ext.FUNCS)
    restypes = {'int': ctypes.c_int, 'longlong': ctypes.c_longlong}
    for ret, name, params in found:
        fn = getattr(_lib.lib, name)
        nargs = 0 if params.strip() == 'void' else params.count(',') + 1
        assert len(fn.argtypes) == nargs == len(_abi_ext.FUNCS[name][1]) == len(_lib._SIGS[name]), name
        assert fn.restype is restypes[ret.replace(' ', '')], name
    assert not set(_abi_ext.FUNCS) & set(_abi.FUNCS)
    assert _abi_ext.CONSTS == _gen_abi().consts(_ext_header())
    for k, v in list(_abi.CONSTS.items()) + list(_abi_ext.CONSTS.items()):
        assert _lib.CONSTS[k] == v
    assert len(_lib.FUNCS) == len(_abi.FUNCS) + len(ENTRY_POINTS) and len(_lib.CONSTS) == len(_abi.CONSTS) + len(_abi_ext.CONSTS)
    assert subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_abi.py'), '--check']).returncode == 0
    for name in ENTRY_POINTS:                                                    # not plan operations: the operation ids do not move
        assert _lib.lib.nele_plan_op_id(name.encode()) == -1


def test_check_mode_covers_each_generated_file(tmp_path):
    """gen_abi.py --check fails when _abi_ext.py alone is stale, when _abi.py alone is and when plan_ops.inc alone is; the tool then
    writes all three back as the tree has them (run on a copy of the tree's inputs and outputs)"""
    for rel in ('tools/gen_abi.py', 'include/nele_hip.h', 'include/nele_hip_ext.h') + GENERATED:
        os.makedirs(os.path.dirname(str(tmp_path / rel)), exist_ok=True)
        shutil.copy(os.path.join(ROOT, rel), str(tmp_path / rel))
    tool = str(tmp_path / 'tools' / 'gen_abi.py')
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 0
    for stale in ('nele_gan_amd/_abi_ext.py', 'nele_gan_amd/_abi.py', 'nele_gan_amd/csrc/plan_ops.inc'):
        with open(str(tmp_path / stale), 'a') as f:
            f.write('# stale\n' if stale.endswith('.py') else '// stale\n')
        assert subprocess.run([sys.executable, tool, '--check']).returncode == 1, stale
        assert subprocess.run([sys.executable, tool], stdout=subprocess.DEVNULL).returncode == 0
        assert subprocess.run([sys.executable, tool, '--check']).returncode == 0, stale
        for rel in GENERATED:
            assert open(str(tmp_path / rel)).read() == open(os.path.join(ROOT, rel)).read(), rel
    os.remove(str(tmp_path / 'nele_gan_amd' / '_abi_ext.py'))                    # a missing file is a stale one
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 1
