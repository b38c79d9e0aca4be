"""CPU: the sixth header include/nele_hip_ext5.h as a whole - it declares exactly the three entry points of the SII-optimal rule and
none of an earlier header's, both libraries export them, nele_gan_amd/_lib.py binds them with the header's arity and constants in dicts
of their own (the earlier headers' dicts and _SIGS keep their sizes), and tools/gen_abi.py --check notices a stale _abi_ext5.py - and,
in a tree without the sixth header, writes and checks what it did before.  Then the entry points themselves without a GPU: bad
arguments rejected with the function's name, and the Python classes' own argument checks."""
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
ENTRY_POINTS = ('nele_siiopt_mask', 'nele_rt_rule_hop', 'nele_rt_rule_finish')
EARLIER_HEADERS = ('nele_hip.h', 'nele_hip_ext.h', 'nele_hip_ext2.h', 'nele_hip_ext3.h', 'nele_hip_ext4.h')
EARLIER = ('nele_gan_amd/_abi.py', 'nele_gan_amd/_abi_ext.py', 'nele_gan_amd/_abi_ext2.py', 'nele_gan_amd/_abi_ext3.py',
           'nele_gan_amd/_abi_ext4.py', 'nele_gan_amd/csrc/plan_ops.inc')
SIXTH = 'nele_gan_amd/_abi_ext5.py'


def _gen_abi():
    spec = importlib.util.spec_from_file_location('gen_abi', os.path.join(ROOT, 'tools', 'gen_abi.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _header(name='nele_hip_ext5.h'):
    return open(os.path.join(ROOT, 'include', name)).read()


def test_the_sixth_header_declares_the_three_entry_points_and_none_of_an_earlier_header():
    gen = _gen_abi()
    src = _header()
    protos = {p[0]: p for p in gen.prototypes(src)}                              # (raises unless every nele_* name is read as one prototype)
    assert sorted(protos) == sorted(ENTRY_POINTS) and len(set(ENTRY_POINTS)) == 3
    consts = gen.consts(src)
    assert consts == {'NELE_SIIOPT_LAMBDA': 0.98, 'NELE_SIIOPT_NMIN': 1e-30, 'NELE_SIIOPT_LOGMAX': 3.2}
    assert protos['nele_siiopt_mask'][3] == ['cb', 'nb', 'gamma', 'B', 'T', 'lam', 'strength', 'mask', 'stream']
    # nele_rt_hop's / nele_rt_finish's arguments without `precision`, with gamma, lam and strength in its place
    rt = {p[0]: p for p in gen.prototypes(_header('nele_hip.h'))}
    for rule, gen_name in (('nele_rt_rule_hop', 'nele_rt_hop'), ('nele_rt_rule_finish', 'nele_rt_finish')):
        names, types = list(rt[gen_name][3]), list(rt[gen_name][2])
        k = names.index('precision')
        assert protos[rule][3] == names[:k] + ['gamma', 'lam', 'strength'] + names[k + 1:]
        assert protos[rule][2] == types[:k] + ['const double*', 'double', 'double'] + types[k + 1:]
    opening = src[:src.index('#ifndef')]
    assert all(name in opening for name in EARLIER_HEADERS)
    for earlier in EARLIER_HEADERS:
        assert not set(ENTRY_POINTS) & set(re.findall(r'\b(nele_[a-z0-9_]+)\s*\(', _header(earlier))), earlier
        assert not set(consts) & set(gen.consts(_header(earlier))), earlier


def test_both_libraries_export_every_entry_point_of_the_sixth_header():
    for name in ('libnele_hip.so', 'libnele_hip_ab.so'):
        lib = ctypes.CDLL(os.path.join(ROOT, 'nele_gan_amd', name))
        assert [s for s in ENTRY_POINTS if not hasattr(lib, s)] == [], name


def test_the_binding_has_the_headers_arity_and_constants_in_dicts_of_their_own():
    from nele_gan_amd import _abi, _abi_ext, _abi_ext2, _abi_ext3, _abi_ext4, _abi_ext5, _lib
    src = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    found = re.findall(r'^([a-z][a-z *]*?)\s*\b(nele_[A-Za-z0-9_]+)\s*\(([^)]*)\)\s*;', src, flags=re.M)      # read here, not by the generator
    assert sorted(f[1] for f in found) == sorted(ENTRY_POINTS) == sorted(_abi_ext5.FUNCS) == sorted(_lib.FUNCS5) == sorted(_lib._SIGS5)
    for ret, name, params in found:
        fn = getattr(_lib.lib, name)
        nargs = params.count(',') + 1
        assert len(fn.argtypes) == nargs == len(_abi_ext5.FUNCS[name][1]) == len(_lib._SIGS5[name]), name
        assert ret.strip() == 'int' and fn.restype is ctypes.c_int, name
    earlier = set(_abi.FUNCS) | set(_abi_ext.FUNCS) | set(_abi_ext2.FUNCS) | set(_abi_ext3.FUNCS) | set(_abi_ext4.FUNCS)
    assert not set(_abi_ext5.FUNCS) & earlier
    assert not set(_lib.FUNCS5) & (set(_lib.FUNCS) | set(_lib.FUNCS2) | set(_lib.FUNCS3) | set(_lib.FUNCS4))
    assert not set(_lib._SIGS5) & (set(_lib._SIGS) | set(_lib._SIGS3) | set(_lib._SIGS4))
    assert _abi_ext5.CONSTS == _gen_abi().consts(_header()) == _lib.CONSTS5
    assert not set(_lib.CONSTS5) & (set(_lib.CONSTS) | set(_lib.CONSTS2) | set(_lib.CONSTS3) | set(_lib.CONSTS4))
    # every size the five earlier ABI tests count is what it was
    assert len(_lib.FUNCS) == len(_abi.FUNCS) + len(_abi_ext.FUNCS) and len(_lib.CONSTS) == len(_abi.CONSTS) + len(_abi_ext.CONSTS)
    assert len(_lib.FUNCS2) == len(_abi_ext2.FUNCS) == 8 and len(_lib._SIGS) == len(_lib.FUNCS) + 8
    assert len(_lib.FUNCS3) == len(_abi_ext3.FUNCS) == len(_lib._SIGS3) == 7
    assert len(_lib.FUNCS4) == len(_abi_ext4.FUNCS) == len(_lib._SIGS4) == 5
    for name in ENTRY_POINTS:                                                    # not plan operations: the operation ids do not move
        assert _lib.lib.nele_plan_op_id(name.encode()) == -1


def _copy(tmp_path, rels):
    for rel in rels:
        os.makedirs(os.path.dirname(str(tmp_path / rel)), exist_ok=True)
        shutil.copy(os.path.join(ROOT, rel), str(tmp_path / rel))
    return str(tmp_path / 'tools' / 'gen_abi.py')


def test_check_mode_notices_a_stale_sixth_file(tmp_path):
    tool = _copy(tmp_path, ('tools/gen_abi.py',) + tuple('include/' + h for h in EARLIER_HEADERS) + ('include/nele_hip_ext5.h',) + EARLIER + (SIXTH,))
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 0
    with open(str(tmp_path / SIXTH), 'a') as f:
        f.write('# stale\n')
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 1
    assert subprocess.run([sys.executable, tool], stdout=subprocess.DEVNULL).returncode == 0
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 0
    for rel in EARLIER + (SIXTH,):
        assert open(str(tmp_path / rel)).read() == open(os.path.join(ROOT, rel)).read(), rel
    os.remove(str(tmp_path / SIXTH))                                             # a missing file is a stale one
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 1
    assert subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_abi.py'), '--check']).returncode == 0       # the tree itself


def test_a_tree_without_the_sixth_header_is_written_and_checked_as_before(tmp_path):
    tool = _copy(tmp_path, ('tools/gen_abi.py',) + tuple('include/' + h for h in EARLIER_HEADERS) + EARLIER)
    assert subprocess.run([sys.executable, tool, '--check']).returncode == 0
    res = subprocess.run([sys.executable, tool], stdout=subprocess.PIPE, universal_newlines=True)
    assert res.returncode == 0 and '_abi_ext4.py (5 entry points)' in res.stdout and '_abi_ext5' not in res.stdout
    assert not os.path.exists(str(tmp_path / SIXTH))
    for rel in EARLIER:
        assert open(str(tmp_path / rel)).read() == open(os.path.join(ROOT, rel)).read(), rel


# ------------------------------------------------------------------------------------------------------- the entry points, no GPU
def _lib():
    from nele_gan_amd import _lib
    return _lib.lib


def test_bad_arguments_are_rejected_without_a_gpu():
    lib = _lib()
    B = 4
    need = lib.nele_rt_state_bytes(B)
    fake = ctypes.c_void_p(1 << 20)                                 # never dereferenced: every call below fails its checks first
    odd = ctypes.c_void_p((1 << 20) + 16)
    nan = float('nan')

    def mask(cb=fake, nb=fake, gamma=fake, B=2, T=3, lam=0.98, s=0.5, out=fake):
        return lib.nele_siiopt_mask(cb, nb, gamma, B, T, lam, s, out, None)

    def hop(state=fake, nbytes=need, S=B, gamma=fake, lam=0.98, s=0.5, clean=fake, noise=fake, nh=1, out=fake, dbg=None, frames=0):
        return lib.nele_rt_rule_hop(state, LL(nbytes), S, gamma, lam, s, clean, noise, None, nh, None, out, None, None, dbg, None, frames, None)

    def finish(state=fake, nbytes=need, S=B, gamma=fake, lam=0.98, s=0.5, tail=fake, lens=fake, out=fake):
        return lib.nele_rt_rule_finish(state, LL(nbytes), S, gamma, lam, s, tail, tail, lens, None, out, None, None, None, None, 0, None)

    cases = [
        (lambda: mask(cb=None), b'nele_siiopt_mask', b'null cb'),
        (lambda: mask(out=None), b'nele_siiopt_mask', b'mask'),
        (lambda: mask(gamma=None), b'nele_siiopt_mask', b'gamma'),
        (lambda: mask(B=0), b'nele_siiopt_mask', b'B=0'),
        (lambda: mask(T=0), b'nele_siiopt_mask', b'T=0'),
        (lambda: mask(B=1 << 20, T=1 << 20), b'nele_siiopt_mask', b'2^31'),
        (lambda: mask(lam=1.0), b'nele_siiopt_mask', b'lam'),
        (lambda: mask(lam=-0.1), b'nele_siiopt_mask', b'lam'),
        (lambda: mask(lam=nan), b'nele_siiopt_mask', b'lam'),
        (lambda: mask(s=0.0), b'nele_siiopt_mask', b'strength'),
        (lambda: mask(s=1.5), b'nele_siiopt_mask', b'strength'),
        (lambda: mask(s=nan), b'nele_siiopt_mask', b'strength'),
        (lambda: hop(state=None), b'nele_rt_rule_hop', b'state'),
        (lambda: hop(nbytes=need - 1), b'nele_rt_rule_hop', b'nele_rt_state_bytes'),
        (lambda: hop(S=0), b'nele_rt_rule_hop', b'max_streams'),
        (lambda: hop(state=odd), b'nele_rt_rule_hop', b'256-byte aligned'),
        (lambda: hop(gamma=None), b'nele_rt_rule_hop', b'gamma'),
        (lambda: hop(lam=1.0), b'nele_rt_rule_hop', b'lam'),
        (lambda: hop(s=0.0), b'nele_rt_rule_hop', b'strength'),
        (lambda: hop(clean=None), b'nele_rt_rule_hop', b'null clean'),
        (lambda: hop(out=None), b'nele_rt_rule_hop', b'out'),
        (lambda: hop(nh=0), b'nele_rt_rule_hop', b'nh'),
        (lambda: hop(dbg=fake, frames=0), b'nele_rt_rule_hop', b'dbg_frames'),
        (lambda: finish(state=None), b'nele_rt_rule_finish', b'state'),
        (lambda: finish(nbytes=need - 1), b'nele_rt_rule_finish', b'nele_rt_state_bytes'),
        (lambda: finish(gamma=None), b'nele_rt_rule_finish', b'gamma'),
        (lambda: finish(s=nan), b'nele_rt_rule_finish', b'strength'),
        (lambda: finish(tail=None), b'nele_rt_rule_finish', b'clean_tail'),
        (lambda: finish(lens=None), b'nele_rt_rule_finish', b'tail_lengths'),
    ]
    for i, (fn, name, what) in enumerate(cases):
        assert fn() == -1, (i, name, what)
        msg = lib.nele_last_error_string()
        assert name in msg and what in msg, (i, msg)


def test_the_rule_adds_no_bytes_to_a_streams_record():
    """Sbar [64] lives where the generator's first history ring does: the record and the state buffer are the sizes they were"""
    lib = _lib()
    rec = lib.nele_rt_stream_record_bytes()
    assert lib.nele_rt_state_bytes(3) - lib.nele_rt_state_bytes(2) == rec
    src = open(os.path.join(ROOT, 'nele_gan_amd', 'csrc', 'realtime.hip')).read()
    assert 'RT_O_SBAR = rt_act_off(1)' in src and 'RT_REC_BYTES = slot_al(rt_y_off(6))' in src


def test_python_classes_reject_bad_settings_before_touching_a_device():
    import numpy as np
    from nele_gan_amd.realtime import RealtimeEnhancer
    from nele_gan_amd.siiopt import SiiOptRule, band_importance
    for kw, what in (({'strength': 0.0}, 'strength'), ({'strength': 1.01}, 'strength'), ({'strength': float('nan')}, 'strength'),
                     ({'lam': 1.0}, 'lam'), ({'lam': -0.01}, 'lam'), ({'importance': np.ones(63)}, 'importance'),
                     ({'importance': -np.ones(64)}, 'importance'), ({'importance': np.zeros(64)}, 'importance'),
                     ({'importance': np.full(64, np.nan)}, 'importance')):
        with pytest.raises(ValueError, match=what):
            SiiOptRule(**kw)
    rule = SiiOptRule()
    assert rule.strength == 0.5 and rule.lam == 0.98 and list(rule.parameters()) == []
    assert np.array_equal(rule.importance, band_importance())
    with pytest.raises(ValueError, match='rule'):
        RealtimeEnhancer(chkpt_path='nowhere.pt', rule=rule)
    with pytest.raises(ValueError, match='rule'):
        RealtimeEnhancer(G=object(), rule=rule)
    with pytest.raises(ValueError, match='SiiOptRule'):
        RealtimeEnhancer(rule=object())
    with pytest.raises(ValueError, match='streams'):
        RealtimeEnhancer(rule=rule, streams=0)
    from nele_gan_amd import inference, siiopt
    assert 'siiopt' in inference.BASELINES
    with pytest.raises(ValueError, match='noise_path'):
        inference.baseline_files('siiopt', [], '/nonexistent')
    with pytest.raises(SystemExit):
        inference.main(['--rule', 'siiopt', '--chkpt', 'x.pt', '--clean', 'a', '--noise', 'b'])
    with pytest.raises(SystemExit):
        siiopt.main(['--clean', 'a', '--noise', 'b', '--out', 'c', '--strength', '2'])
    from nele_gan_amd.train_nele import GanTrainer
    with pytest.raises(ValueError, match='train_enh_path'):
        GanTrainer.fit(object(), [], None, multienh='siiopt', train_enh_path='x')
