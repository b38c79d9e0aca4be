"""CPU: the 'bf16x3' precision's interface - the split entry points in the header, the library and the Python binding, and the command
lines that accept the new precision (no GPU needed)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('nele_weight_prep_frag16x3', 'nele_weight_prep_frag16x3_batch', 'nele_conv_span_bf16x3', 'nele_conv_span_bf16x3_supported',
       'nele_conv_wgrad_bf16x3', 'nele_conv_wgrad_bf16x3_supported')


def test_split_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, 'include', 'nele_hip.h')).read()
    assert re.search(r'#define\s+NELE_PREC_F32\s+0\b', hdr)
    assert re.search(r'#define\s+NELE_PREC_BF16\s+1\b', hdr)
    assert re.search(r'#define\s+NELE_PREC_BF16X3\s+2\b', hdr)
    lib = ctypes.CDLL(os.path.join(ROOT, 'nele_gan_amd', 'libnele_hip.so'))
    from nele_gan_amd import _lib, ops  # noqa: F401
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, hdr), name
        assert hasattr(lib, name), name
        assert name in _lib._SIGS, name
    ops_inc = open(os.path.join(ROOT, 'nele_gan_amd', 'csrc', 'plan_ops.inc')).read()
    for name in ('nele_weight_prep_frag16x3_batch', 'nele_conv_span_bf16x3', 'nele_conv_wgrad_bf16x3'):
        assert re.search(r'PLAN_OP\(\d+, %s,' % name, ops_inc), name


def test_workspace_sizes_take_the_precision_code():
    """codes 0 and 1 keep their sizes; 2 (bf16x3) adds the hi / lo fragment streams to the float32 layout; other nonzero codes mean bf16"""
    from nele_gan_amd import _lib
    L = _lib.lib
    g = [int(L.nele_gen_workspace_bytes(8, 251, p, 1)) for p in (0, 1, 2, 7)]
    d = [int(L.nele_disc_workspace_bytes(8, 251, 3, p)) for p in (0, 1, 2, 7)]
    assert g[3] == g[1] and d[3] == d[1]
    assert g[2] > g[0] and d[2] > d[0]


def _main_gets_past_argparse(fn, argv):
    try:
        fn(argv)
    except SystemExit as e:
        assert e.code != 2, 'argparse refused %s' % argv
    except Exception:                                       # the missing checkpoint / corpus or the missing GPU, after parsing
        pass


def test_inference_cli_accepts_bf16x3(tmp_path):
    from nele_gan_amd import inference
    missing = str(tmp_path / 'missing')
    _main_gets_past_argparse(inference.main, ['--chkpt', missing + '.pt', '--clean', missing, '--noise', missing, '--output', str(tmp_path / 'out'),
                                              '--precision', 'bf16x3'])


def test_train_cli_accepts_bf16x3(tmp_path):
    from nele_gan_amd import train_nele
    missing = str(tmp_path / 'missing')
    _main_gets_past_argparse(train_nele.main, ['--data', missing, '--resume', missing + '.pt', '--output', str(tmp_path / 'o'), '--chkpt',
                                               str(tmp_path / 'c'), '--log', str(tmp_path / 'log.txt'), '--precision', 'bf16x3'])
