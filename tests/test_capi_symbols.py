"""CPU: libnele_hip.so loads (no GPU needed) and exports every symbol include/nele_hip.h declares."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, 'include', 'nele_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(nele_[A-Za-z0-9_]+)\s*\(', src)))


def test_header_declares_entry_points():
    syms = declared_symbols()
    for must in ('nele_version', 'nele_last_error_string', 'nele_stft_band', 'nele_imcra_band', 'nele_gain_istft'):
        assert must in syms


def test_library_exports_every_declared_symbol():
    path = os.path.join(ROOT, 'nele_gan_amd', 'libnele_hip.so')
    assert os.path.exists(path), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(path)
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    assert not missing, "declared in include/nele_hip.h but not exported: %s" % missing
    lib.nele_version.restype = ctypes.c_int
    assert lib.nele_version() >= 100


def test_python_binding_covers_header():
    from nele_gan_amd import _lib
    bound = set(_lib._SIGS) | {'nele_version', 'nele_last_error_string'}
    assert set(declared_symbols()) <= bound, sorted(set(declared_symbols()) - bound)


def test_invalid_arguments_are_reported_without_a_gpu():
    from nele_gan_amd import _lib
    st = _lib.lib.nele_stft_band(None, 0, 0, 0.0, None, None, None)
    assert st == -1
    assert b'nele_stft_band' in _lib.lib.nele_last_error_string()


def test_product_library_has_no_switches_and_the_test_library_exports_the_same_abi():
    """libnele_hip.so (product): NELE_* environment switches are compile-time constants, the superseded kernel variants are not built.
    libnele_hip_ab.so (tests / tools, -DNELE_AB): same sources, same exported symbols, switches read from the environment."""
    prod = ctypes.CDLL(os.path.join(ROOT, 'nele_gan_amd', 'libnele_hip.so'))
    ab_path = os.path.join(ROOT, 'nele_gan_amd', 'libnele_hip_ab.so')
    assert os.path.exists(ab_path), "make -C nele_gan_amd/csrc builds both libraries"
    ab = ctypes.CDLL(ab_path)
    assert prod.nele_build_has_ab_switches() == 0 and ab.nele_build_has_ab_switches() == 1
    missing = [s for s in declared_symbols() if not hasattr(ab, s)]
    assert not missing, missing
    # no getenv in the product library's import table
    import subprocess
    nm = subprocess.run(['nm', '-D', '--undefined-only', os.path.join(ROOT, 'nele_gan_amd', 'libnele_hip.so')], stdout=subprocess.PIPE, text=True).stdout
    assert 'getenv' not in nm
    nm_ab = subprocess.run(['nm', '-D', '--undefined-only', ab_path], stdout=subprocess.PIPE, text=True).stdout
    assert 'getenv' in nm_ab


def _gen_abi():
    import importlib.util
    spec = importlib.util.spec_from_file_location('gen_abi', os.path.join(ROOT, 'tools', 'gen_abi.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plan_operation_table_is_generated_from_the_header():
    """csrc/plan_ops.inc (the dispatch table of nele_plan_run) and nele_gan_amd/_abi.py (what _lib.py binds) are generated from
    include/nele_hip.h by tools/gen_abi.py."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_abi.py'), '--check'])
    assert r.returncode == 0, "include/nele_hip.h changed: run python tools/gen_abi.py and rebuild"
    from nele_gan_amd import _lib
    for name in ('nele_conv16', 'nele_glayer16_fwd', 'nele_cln_bwd', 'nele_event_record', 'nele_vec_add', 'nele_gap_mlp_bwd_var16'):
        op = _lib.lib.nele_plan_op_id(name.encode())
        assert op >= 0 and _lib.lib.nele_plan_op_nargs(op) == len(_lib._SIGS[name]), name
    assert _lib.lib.nele_plan_op_id(b'nele_version') == -1


def declared_prototypes():
    """name -> (return type, number of parameters) of every prototype of the header, read here and not by the generator's parser"""
    src = open(os.path.join(ROOT, 'include', 'nele_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    out = {}
    for ret, name, params in re.findall(r'^([a-z][a-z *]*?)\s*\b(nele_[A-Za-z0-9_]+)\s*\(([^)]*)\)\s*;', src, flags=re.M):
        out[name] = (ret.replace(' ', ''), 0 if params.strip() == 'void' else params.count(',') + 1)
    return out


def test_every_entry_point_is_bound_with_the_headers_arity_and_return_type():
    from nele_gan_amd import _abi, _lib
    protos = declared_prototypes()
    assert len(protos) == 200 and sorted(protos) == declared_symbols() == sorted(_abi.FUNCS)
    restypes = {'int': ctypes.c_int, 'longlong': ctypes.c_longlong, 'constchar*': ctypes.c_char_p, 'float*': ctypes.c_void_p,
                'void*': ctypes.c_void_p}
    for name, (ret, nargs) in protos.items():
        fn = getattr(_lib.lib, name)
        assert len(fn.argtypes) == nargs == len(_abi.FUNCS[name][1]) == len(_lib._SIGS[name]), name
        assert fn.restype is restypes[ret], name


SYNTHETIC_HEADER = '''
#ifndef NELE_SYNTH_H
#define NELE_SYNTH_H
#define NELE_A 24
#define NELE_B (1 << 30)   /* a comment */
#define NELE_C 0.5
#define NELE_D -3
#define NELE_E 1e3
typedef struct nele_rec { int a[NELE_A]; double b; } nele_rec;
int nele_scalars(int a, unsigned b, long long c, unsigned long long d, float e, double f);
int nele_pointers(const char* name, char* buf, const float* x, void* const* streams_host, const char* const* paths,
                  const nele_rec* rec, const unsigned char* mask /* or NULL */, short* pcm);
long long nele_bytes(int B);
void* nele_buffer(void* ws);
float* nele_floats(void* ws);
const char* nele_text(void);
int nele_nothing(void);
int nele_band_E(int N);
#endif
'''


def test_the_generators_type_map():
    gen = _gen_abi()
    assert gen.funcs(SYNTHETIC_HEADER) == {
        'nele_scalars': ('int', ('int', 'uint', 'longlong', 'ulonglong', 'float', 'double')),
        'nele_pointers': ('int', ('char_p', 'void_p', 'void_p', 'void_p', 'void_p', 'void_p', 'void_p', 'void_p')),
        'nele_bytes': ('longlong', ('int',)),
        'nele_buffer': ('void_p', ('void_p',)),
        'nele_floats': ('void_p', ('void_p',)),
        'nele_text': ('char_p', ()),
        'nele_nothing': ('int', ()),
        'nele_band_E': ('int', ('int',)),
    }
    assert gen.consts(SYNTHETIC_HEADER) == {'NELE_A': 24, 'NELE_B': 1 << 30, 'NELE_C': 0.5, 'NELE_D': -3, 'NELE_E': 1000.0}
    for bad in ('int nele_f(size_t n);', 'int nele_f(int a, short b);', 'short nele_f(int a);', 'void nele_f(int a);', 'int nele_f(unsigned int a);',
                'int nele_f(void (*callback)(int), int n);', 'int nele_f(int a); int nele_f(int a);'):
        with pytest.raises(ValueError, match='nele_f'):
            gen.funcs(bad)
    for bad in ('#define NELE_X (NELE_A + 1)', '#define NELE_X sizeof(int)', '#define NELE_X(a) 1', '#define NELE_X "text"'):
        with pytest.raises(ValueError, match='NELE_X'):
            gen.consts(bad)


def test_constants_come_from_the_header():
    from nele_gan_amd import _abi, _lib
    hdr = open(os.path.join(ROOT, 'include', 'nele_hip.h')).read()
    for name, value in (('NELE_PLAN_MAXARGS', 24), ('NELE_SSDRC_MAX_KNOTS', 8), ('NELE_RESAMPLE_MAX_SAMPLES', 1 << 30), ('NELE_P56_NO_CROSSING', 4),
                        ('NELE_RIR_BAD_BETA', 4)):
        digits, shift = re.search(r'^#define %s (?:(\d+)|\(1 << (\d+)\))' % name, hdr, flags=re.M).groups()
        assert _abi.CONSTS[name] == value == (int(digits) if digits else 1 << int(shift)), name
    assert ctypes.sizeof(_lib.nele_plan_job) == 16 + 20 * _abi.CONSTS['NELE_PLAN_MAXARGS']


def test_no_module_but_lib_declares_a_signature():
    pkg = os.path.join(ROOT, 'nele_gan_amd')
    files = [os.path.join(d, f) for d, _, fs in os.walk(pkg) for f in fs if f.endswith('.py')]
    assert len(files) > 20
    for path in files:
        if path != os.path.join(pkg, '_lib.py'):
            text = open(path).read()
            for needle in ('.argtypes', '.restype', 'declare('):
                assert needle not in text, "%s contains %r: signatures come from _abi.py through _lib.py alone" % (path, needle)
