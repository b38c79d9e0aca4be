#!/usr/bin/env python
"""Generates, from include/nele_hip.h (the contract of libnele_hip.so), the two files that restate it:
  nele_gan_amd/csrc/plan_ops.inc   one `case` per entry point whose last parameter is the stream, for the job-table executor of
                                   csrc/plan.hip (nele_plan_run);
  nele_gan_amd/_abi.py             FUNCS (name -> restype code, argtype codes: what nele_gan_amd/_lib.py binds through ctypes) and CONSTS
                                   (the header's numeric #define NELE_* values);
and from include/nele_hip_ext.h (the entry points added after nele_hip.h's fixed set; same parser, same type map)
  nele_gan_amd/_abi_ext.py         FUNCS and CONSTS of that header, bound by _lib.py beside _abi.py's.  None of them is a plan operation:
                                   plan_ops.inc and the operation ids come from nele_hip.h alone.
and, when the tree has it, from include/nele_hip_ext2.h (the entry points added after nele_hip_ext.h's fixed set)
  nele_gan_amd/_abi_ext2.py        FUNCS and CONSTS of that header, bound by _lib.py into dicts of their own.  A tree without the header
                                   gets, and is checked for, the three files above only.
and, when the tree has it, from include/nele_hip_ext3.h (the entry points added after nele_hip_ext2.h's fixed set)
  nele_gan_amd/_abi_ext3.py        likewise, into dicts of their own again; a tree without that header is written and checked without it.
and, when the tree has it, from include/nele_hip_ext4.h (the entry points added after nele_hip_ext3.h's fixed set)
  nele_gan_amd/_abi_ext4.py        likewise.
and, when the tree has it, from include/nele_hip_ext5.h (the entry points added after nele_hip_ext4.h's fixed set)
  nele_gan_amd/_abi_ext5.py        likewise.
and, when the tree has it, from include/nele_hip_ext6.h (the entry points added after nele_hip_ext5.h's fixed set)
  nele_gan_amd/_abi_ext6.py        likewise.
and, when the tree has it, from include/nele_hip_ext7.h (the entry points added after nele_hip_ext6.h's fixed set)
  nele_gan_amd/_abi_ext7.py        likewise.
and, when the tree has it, from include/nele_hip_ext8.h (the entry points added after nele_hip_ext7.h's fixed set)
  nele_gan_amd/_abi_ext8.py        likewise.
and, when the tree has it, from include/nele_hip_ext9.h (the entry points added after nele_hip_ext8.h's fixed set)
  nele_gan_amd/_abi_ext9.py        likewise.
and, when the tree has it, from include/nele_hip_ext10.h (the entry points added after nele_hip_ext9.h's fixed set)
  nele_gan_amd/_abi_ext10.py       likewise.
Run after changing a header; tests/test_capi_symbols.py, tests/test_abi_ext_cpu.py, tests/test_abi_ext2_cpu.py,
tests/test_abi_ext3_cpu.py, tests/test_abi_ext4_cpu.py, tests/test_abi_ext5_cpu.py, tests/test_abi_ext6_cpu.py, tests/test_abi_ext7_cpu.py, tests/test_abi_ext8_cpu.py, tests/test_abi_ext9_cpu.py and tests/test_abi_ext10_cpu.py check that
all are current.
    python tools/gen_abi.py            # rewrite the files
    python tools/gen_abi.py --check    # exit 1 when a committed file differs
A code is the ctypes type's name without its 'c_'.  The map is fixed: a scalar type outside it stops the tool (never a default)."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_PLAN_OPS = ('nele_compute_band_E',)     # never in the table (the table's first generator skipped the capital); kept out so that the
                                             # operation ids of a built library stay as they are
SCALARS = {'int': 'int', 'unsigned': 'uint', 'long long': 'longlong', 'unsigned long long': 'ulonglong', 'float': 'float',
           'double': 'double'}


def _header(name='nele_hip.h'):
    return open(os.path.join(ROOT, 'include', name)).read()


def _strip_comments(src):
    return re.sub(r'/\*.*?\*/', '', src, flags=re.S)


def prototypes(src=None):
    """-> sorted [(name, return type, [parameter types], [parameter names])] of every `nele_*` prototype of the header text, the types as
    written (blanks collapsed); `(void)` gives no parameters."""
    src = re.sub(r'^[ \t]*#.*$', '', _strip_comments(_header() if src is None else src), flags=re.M)
    out = []
    for m in re.finditer(r'([A-Za-z_][A-Za-z0-9_ \t\n*]*?)\b(nele_[A-Za-z0-9_]+)\s*\(([^;{()]*)\)\s*;', src):
        ret, name, params = ' '.join(m.group(1).split()), m.group(2), ' '.join(m.group(3).split())
        ps = [] if params in ('void', '') else [p.strip() for p in params.split(',')]
        types = [re.sub(r'\b[A-Za-z_][A-Za-z0-9_]*$', '', p).strip() for p in ps]      # drop the parameter name
        out.append((name, ret, types, [p[len(t):].strip() for p, t in zip(ps, types)]))
    unread = sorted(set(re.findall(r'\b(nele_[A-Za-z0-9_]+)\s*\(', src)) - {p[0] for p in out})
    if unread or len({p[0] for p in out}) != len(out):
        raise ValueError("not read as one prototype each: %s" % (unread or sorted(p[0] for p in out)))
    return sorted(out)


def code(ctype, where):
    """C type -> ctypes code; `where` names the prototype in the error."""
    words = [w for w in ctype.replace('*', ' * ').split() if w != 'const']
    if '*' in words:
        return 'char_p' if words == ['char', '*'] and ctype.lstrip().startswith('const') else 'void_p'
    if ' '.join(words) not in SCALARS:
        raise ValueError("%s: no ctypes type for '%s'" % (where, ctype))
    return SCALARS[' '.join(words)]


def funcs(src=None):
    """-> {name: (restype code, (argtype codes))}"""
    return {name: (code(ret, name), tuple(code(t, name) for t in types)) for name, ret, types, _ in prototypes(src)}


def consts(src=None):
    """-> {NELE_*: value} of the header's #defines: integer and floating literals and (1 << N); a macro without a body (the include guard)
    is none of them and is left out."""
    src = _strip_comments(_header() if src is None else src)
    out = {}
    for m in re.finditer(r'^[ \t]*#[ \t]*define[ \t]+(NELE_[A-Za-z0-9_]+)(.*)$', src, flags=re.M):
        name, body = m.group(1), m.group(2).strip()
        if not body:
            continue
        shift = re.match(r'^\(\s*1\s*<<\s*(\d+)\s*\)$', body)
        if shift:
            out[name] = 1 << int(shift.group(1))
        elif re.match(r'^[-+]?(\d+|0[xX][0-9a-fA-F]+)$', body):
            out[name] = int(body, 0)
        elif re.match(r'^[-+]?(\d+\.\d*|\.\d+|\d+)([eE][-+]?\d+)?$', body):
            out[name] = float(body)
        else:
            raise ValueError("#define %s: '%s' is not a numeric literal" % (name, body))
    return out


def plan_operations():
    """The prototypes nele_plan_run dispatches: status-returning, enqueueing on a stream (their last parameter)."""
    out, maxargs = [], consts()['NELE_PLAN_MAXARGS']
    for name, ret, types, names in prototypes():
        if (ret != 'int' or not types or (types[-1], names[-1]) != ('void*', 'stream') or name.startswith(('nele_plan_', 'nele_profile'))
                or name in NOT_PLAN_OPS):
            continue
        if len(types) > maxargs:
            raise SystemExit('%s has %d parameters (> %d)' % (name, len(types), maxargs))
        out.append((name, types))
    return out


def emit_plan_ops():
    lines = ['// GENERATED by tools/gen_abi.py from include/nele_hip.h - do not edit.',
             '// PLAN_OP(index, name, nargs) table, then the dispatch cases: V(i) = 64-bit integer / pointer value of argument i, D(i) = its',
             '// floating-point value, S = the job\'s stream.', '#ifdef PLAN_OP_TABLE']
    protos = plan_operations()
    for k, (name, types) in enumerate(protos):
        lines.append('PLAN_OP(%d, %s, %d)' % (k, name, len(types)))
    lines.append('#endif')
    lines.append('#ifdef PLAN_OP_CASES')
    for k, (name, types) in enumerate(protos):
        args = []
        for i, t in enumerate(types[:-1]):
            if '*' in t:
                args.append('(%s)(uintptr_t)V(%d)' % (t, i))
            elif t in ('float', 'double'):
                args.append('(%s)D(%d)' % (t, i))
            else:
                args.append('(%s)V(%d)' % (t, i))
        args.append('S')
        lines.append('case %d: return %s(%s);' % (k, name, ', '.join(args)))
    lines.append('#endif')
    return '\n'.join(lines) + '\n'


def emit_abi(header='nele_hip.h'):
    src = None if header == 'nele_hip.h' else _header(header)
    lines = ['"""GENERATED by tools/gen_abi.py from include/%s - do not edit.' % header,
             'FUNCS: entry point -> (restype, argtypes), each the name of a ctypes type without its \'c_\'; CONSTS: the header\'s #define NELE_*."""',
             'CONSTS = {']
    lines += ['    %r: %r,' % kv for kv in sorted(consts(src).items())]
    lines += ['}', 'FUNCS = {']
    lines += ['    %r: %r,' % kv for kv in sorted(funcs(src).items())]
    lines.append('}')
    return '\n'.join(lines) + '\n'


if __name__ == '__main__':
    outputs = ((os.path.join(ROOT, 'nele_gan_amd', 'csrc', 'plan_ops.inc'), emit_plan_ops()),
               (os.path.join(ROOT, 'nele_gan_amd', '_abi.py'), emit_abi()),
               (os.path.join(ROOT, 'nele_gan_amd', '_abi_ext.py'), emit_abi('nele_hip_ext.h')))
    third = os.path.exists(os.path.join(ROOT, 'include', 'nele_hip_ext2.h'))     # a tree without the third header: the three files above only
    if third:
        outputs += ((os.path.join(ROOT, 'nele_gan_amd', '_abi_ext2.py'), emit_abi('nele_hip_ext2.h')),)
    fourth = os.path.exists(os.path.join(ROOT, 'include', 'nele_hip_ext3.h'))    # likewise
    if fourth:
        outputs += ((os.path.join(ROOT, 'nele_gan_amd', '_abi_ext3.py'), emit_abi('nele_hip_ext3.h')),)
    fifth = os.path.exists(os.path.join(ROOT, 'include', 'nele_hip_ext4.h'))     # likewise
    if fifth:
        outputs += ((os.path.join(ROOT, 'nele_gan_amd', '_abi_ext4.py'), emit_abi('nele_hip_ext4.h')),)
    sixth = os.path.exists(os.path.join(ROOT, 'include', 'nele_hip_ext5.h'))     # likewise
    n_before_sixth = len(outputs)
    if sixth:
        outputs += ((os.path.join(ROOT, 'nele_gan_amd', '_abi_ext5.py'), emit_abi('nele_hip_ext5.h')),)
    seventh = os.path.exists(os.path.join(ROOT, 'include', 'nele_hip_ext6.h'))   # likewise
    n_before_seventh = len(outputs)
    if seventh:
        outputs += ((os.path.join(ROOT, 'nele_gan_amd', '_abi_ext6.py'), emit_abi('nele_hip_ext6.h')),)
    eighth = os.path.exists(os.path.join(ROOT, 'include', 'nele_hip_ext7.h'))    # likewise
    n_before_eighth = len(outputs)
    if eighth:
        outputs += ((os.path.join(ROOT, 'nele_gan_amd', '_abi_ext7.py'), emit_abi('nele_hip_ext7.h')),)
    ninth = os.path.exists(os.path.join(ROOT, 'include', 'nele_hip_ext8.h'))     # likewise
    n_before_ninth = len(outputs)
    if ninth:
        outputs += ((os.path.join(ROOT, 'nele_gan_amd', '_abi_ext8.py'), emit_abi('nele_hip_ext8.h')),)
    tenth = os.path.exists(os.path.join(ROOT, 'include', 'nele_hip_ext9.h'))     # likewise
    n_before_tenth = len(outputs)
    if tenth:
        outputs += ((os.path.join(ROOT, 'nele_gan_amd', '_abi_ext9.py'), emit_abi('nele_hip_ext9.h')),)
    eleventh = os.path.exists(os.path.join(ROOT, 'include', 'nele_hip_ext10.h'))  # likewise
    n_before_eleventh = len(outputs)
    if eleventh:
        outputs += ((os.path.join(ROOT, 'nele_gan_amd', '_abi_ext10.py'), emit_abi('nele_hip_ext10.h')),)
    if '--check' in sys.argv:
        sys.exit(0 if all(os.path.exists(path) and open(path).read() == text for path, text in outputs) else 1)
    for path, text in outputs:
        open(path, 'w').write(text)
    print('wrote %s (%d operations), %s (%d entry points) and %s (%d entry points)'
          % (outputs[0][0], outputs[0][1].count('PLAN_OP('), outputs[1][0], len(funcs()), outputs[2][0], len(funcs(_header('nele_hip_ext.h')))))
    if third:
        print('wrote %s (%d entry points)' % (outputs[3][0], len(funcs(_header('nele_hip_ext2.h')))))
    if fourth:
        print('wrote %s (%d entry points)' % (outputs[:n_before_sixth][-2 if fifth else -1][0], len(funcs(_header('nele_hip_ext3.h')))))
    if fifth:
        print('wrote %s (%d entry points)' % (outputs[n_before_sixth - 1][0], len(funcs(_header('nele_hip_ext4.h')))))
    if sixth:
        print('wrote %s (%d entry points)' % (outputs[n_before_seventh - 1][0], len(funcs(_header('nele_hip_ext5.h')))))
    if seventh:
        print('wrote %s (%d entry points)' % (outputs[n_before_eighth - 1][0], len(funcs(_header('nele_hip_ext6.h')))))
    if eighth:
        print('wrote %s (%d entry points)' % (outputs[n_before_ninth - 1][0], len(funcs(_header('nele_hip_ext7.h')))))
    if ninth:
        print('wrote %s (%d entry points)' % (outputs[n_before_tenth - 1][0], len(funcs(_header('nele_hip_ext8.h')))))
    if tenth:
        print('wrote %s (%d entry points)' % (outputs[n_before_eleventh - 1][0], len(funcs(_header('nele_hip_ext9.h')))))
    if eleventh:
        print('wrote %s (%d entry points)' % (outputs[-1][0], len(funcs(_header('nele_hip_ext10.h')))))
