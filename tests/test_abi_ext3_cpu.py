"""CPU: the fourth header include/nele_hip_ext3.h as a whole - it declares exactly the seven entry points of the scheduled stream
converter and none of an earlier header's, both libraries export them, nele_gan_amd/_lib.py binds them with the header's arity and
constants in dicts of their own (the earlier headers' dicts and _SIGS keep their sizes), and tools/gen_abi.py --check notices a stale
_abi_ext3.py - and, in a tree without the fourth header, writes and checks what it did before."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('nele_sched_stream_plan', 'nele_sched_stream_widths', 'nele_sched_stream_record_bytes', 'nele_sched_stream_state_bytes',
                'nele_sched_stream_init', 'nele_sched_stream_reset', 'nele_sched_stream_hop')
EARLIER_HEADERS = ('nele_hip.h', 'nele_hip_ext.h', 'nele_hip_ext2.h')
EARLIER = ('nele_gan_amd/_abi.py', 'nele_gan_amd/_abi_ext.py', 'nele_gan_amd/_abi_ext2.py', 'nele_gan_amd/csrc/plan_ops.inc')
FOURTH = 'nele_gan_amd/_abi_ext3.py'


def _gen_abi():
    spec = importlib.util.spec_from_file_location('gen_abi', os.path.join(ROOT, 'tools', 'gen_abi.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _header(name='nele_hip_ext3.h'):
    return open(os.path.join(ROOT, 'include', name)).read()


def test_the_fourth_header_declares_the_seven_entry_points_and_none_of_an_earlier_header():
    gen = _gen_abi()
    src = _header()
    protos = {p[0]: p for p in gen.prototypes(src)}                              # (raises unless every nele_* name is read as one prototype)
    assert sorted(protos) == sorted(ENTRY_POINTS) and len(set(ENTRY_POINTS)) == 7
    consts = gen.consts(src)
    assert consts['NELE_SCHED_INFO'] == 9
    assert sorted(v for k, v in consts.items() if k.startswith('NELE_SCHED_I_')) == list(range(9)) and len(consts) == 10
    assert protos['nele_sched_stream_hop'][3] == ['state', 'state_bytes', 'max_streams', 'up', 'down', 'K', 'to16k', 'hp_dev', 'x', 'x_stride',
                                                  'active', 'nh', 'pos', 'y', 'y_stride', 'stream']
    assert protos['nele_sched_stream_plan'][3] == ['up', 'down', 'zeros', 'to16k', 'info_host']
    assert protos['nele_sched_stream_widths'][3] == ['up', 'down', 'to16k', 'pos', 'nh', 'n_in', 'n_out']
    assert protos['nele_sched_stream_reset'][3][-2:] == ['slots', 'stream']
    opening = src[:src.index('#ifndef')]
    assert all(name in opening for name in EARLIER_HEADERS)
    for earlier in EARLIER_HEADERS:
        assert not set(ENTRY_POINTS) & set(re.findall(r'\b(nele_[a-z0-9_]+)\s*\(', _header(earlier))), earlier
        assert not set(consts) & set(gen.consts(_header(earlier))), earlier


def test_both_libraries_export_every_entry_point_of_the_fourth_header():
    for name in ('libnele_hip.so', 'libnele_hip_ab.so'):
        lib = ctypes.CDLL(os.path.join(ROOT, 'nele_gan_amd', name))
        assert [s for s in ENTRY_POINTS if not hasattr(lib, s)] == [], name


def test_the_binding_has_the_headers_arity_and_constants_in_dicts_of_their_own():
    from nele_gan_amd import _abi, _abi_ext, _abi_ext2, _abi_ext3, _lib
    src = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    found = re.findall(r'^([a-z][a-z *]*?)\s*\b(nele_[A-Za-z0-9_]+)\s*\(([^)]*)\)\s*;', src, flags=re.M)      # read here, not by the generator
    assert sorted(f[1] for f in found) == sorted(ENTRY_POINTS) == sorted(_abi_ext3.FUNCS) == sorted(_lib.FUNCS3) == sorted(_lib._SIGS3)
    restypes = {'int': ctypes.c_int, 'longlong': ctypes.c_longlong}
    for ret, name, params in found:
        fn = getattr(_lib.lib, name)
        nargs = 0 if params.strip() == 'void' else params.count(',') + 1
        assert len(fn.argtypes) == nargs == len(_abi_ext3.FUNCS[name][1]) == len(_lib._SIGS3[name]), name
        assert fn.restype is restypes[ret.replace(' ', '')], name
    earlier = set(_abi.FUNCS) | set(_abi_ext.FUNCS) | set(_abi_ext2.FUNCS)
    assert not set(_abi_ext3.FUNCS) & earlier and not set(_lib.FUNCS3) & (set(_lib.FUNCS) | set(_lib.FUNCS2)) and not set(_lib._SIGS3) & set(_lib._SIGS)
    assert _abi_ext3.CONSTS == _gen_abi().consts(_header()) == _lib.CONSTS3 and not set(_lib.CONSTS3) & (set(_lib.CONSTS) | set(_lib.CONSTS2))
    # every size the three earlier ABI tests count is what it was
    assert len(_lib.FUNCS) == len(_abi.FUNCS) + len(_abi_ext.FUNCS) and len(_lib.CONSTS) == len(_abi.CONSTS) + len(_abi_ext.CONSTS)
    assert len(_lib.FUNCS2) == len(_abi_ext2.FUNCS) == 8 and len(_lib._SIGS) == len(_lib.FUNCS) + 8
    for name in ENTRY_POINTS:                                                    # not plan operations: the operation ids do not move
        assert _lib.lib.nele_plan_op_id(name.encode()) == -1


def _copy(tmp_path, rels):
    for rel in rels:
        os.makedirs(os.path.dirname(str(tmp_path / rel)), exist_ok=True)
        shutil.copy(os.path.join(ROOT, rel), str(tmp_path / rel))
    return str(tmp_path / 'tools' / 'gen_abi.py')


def test_check_mode_notices_a_stale_fourth_file(tmp_path):
    tool = _copy(tmp_path, ('tools/gen_abi.py',) + tuple('include/' + h for h in EARLIER_HEADERS) + ('include/nele_hip_ext3.h',) + EARLIER + (FOURTH,))
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 0
    with open(str(tmp_path / FOURTH), 'a') as f:
        f.write('# stale\n')
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 1
    assert subprocess.run([sys.executable, tool], stdout=subprocess.DEVNULL).returncode == 0
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 0
    for rel in EARLIER + (FOURTH,):
        assert open(str(tmp_path / rel)).read() == open(os.path.join(ROOT, rel)).read(), rel
    os.remove(str(tmp_path / FOURTH))                                            # a missing file is a stale one
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 1
    assert subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_abi.py'), '--check']).returncode == 0       # the tree itself


def test_a_tree_without_the_fourth_header_is_written_and_checked_as_before(tmp_path):
    tool = _copy(tmp_path, ('tools/gen_abi.py',) + tuple('include/' + h for h in EARLIER_HEADERS) + EARLIER)
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 0
    assert subprocess.run([sys.executable, tool], stdout=subprocess.DEVNULL).returncode == 0
    assert not os.path.exists(str(tmp_path / FOURTH))
    for rel in EARLIER:
        assert open(str(tmp_path / rel)).read() == open(os.path.join(ROOT, rel)).read(), rel
