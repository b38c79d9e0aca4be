#!/usr/bin/env python3
"""Writes tests/golden/ws_sections.json: what the host-only workspace functions of the library (the *_workspace_bytes sizes and the
*_sections / *_clean_sections byte ranges) answer at a fixed set of geometries, argument errors included.  No GPU is needed.

    python tools/gen_ws_sections.py [LIB ...]      (default: nele_gan_amd/libnele_hip.so and libnele_hip_ab.so)

Every library given must answer alike; tests/test_ws_sections_cpu.py replays the records against both libraries of a build and compares
value for value, so a change of a workspace layout or of a section list shows as a diff of the fixture."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'ws_sections.json')
LL = ctypes.c_longlong
CAP = 24                                      # sections the replay buffer holds (the caches in metrics.py use the same)
FILL = -7                                     # what the buffer holds before a call: a function writes its sections and nothing else

BS = (1, 50, 130)                             # the three segment classes of SIIB's lag products
LS = (2400, 16000, 64000, 200000)             # HASPI's minimum .. long enough for its chunk length to grow at 16 kHz
FSS = (8000, 16000, 24000)
SIZES = {                                     # name -> number of leading int arguments (B, L[, fs])
    'nele_metric_estoi_workspace_bytes': 2, 'nele_metric_siib_workspace_bytes': 2, 'nele_metric_haspi_workspace_bytes': 3,
    'nele_metric_haspi_quality_workspace_bytes': 3, 'nele_metric_hasqi_workspace_bytes': 3}
SECTIONS = {                                  # name -> (number of leading int arguments, sections of a good call)
    'nele_metric_estoi_sections': (2, 6), 'nele_metric_siib_clean_sections': (2, 13), 'nele_metric_haspi_clean_sections': (3, 16),
    'nele_metric_haspi_sections': (3, 15), 'nele_metric_hasqi_clean_sections': (3, 12), 'nele_metric_siib_sections': (2, 10),
    'nele_metric_haspi_quality_sections': (3, 17)}


def cases():
    """-> [(function, int arguments, max_sections or None for a size function)]"""
    out = []
    geoms = {2: [(B, L) for B in BS for L in LS], 3: [(B, L, fs) for B in BS for L in LS for fs in FSS]}
    for name, na in SIZES.items():
        out += [(name, g, None) for g in geoms[na]]
    out += [('nele_eigh_workspace_bytes', (B, n), None) for B in BS for n in (2, 420, 512)]
    for name, (na, nsec) in SECTIONS.items():
        out += [(name, g, CAP) for g in geoms[na]]
        out.append((name, geoms[na][1], nsec))                    # exactly enough room
        out.append((name, geoms[na][1], nsec - 1))                # one section short: an argument error
        if na == 3:
            out += [(name, (3, 16000, 25000), CAP), (name, (3, 2399, 16000), CAP)]
    for name in ('nele_metric_estoi_workspace_bytes', 'nele_metric_estoi_sections'):
        out += [(name, (B, 100), None if name.endswith('bytes') else CAP) for B in BS]      # no frame at all (F = 0)
    return out


def replay(lib, name, args, cap):
    """One call -> (return value, the triples written) - and the check that nothing behind them was touched."""
    fn = getattr(lib, name)
    if cap is None:
        fn.restype, fn.argtypes = LL, [ctypes.c_int] * len(args)
        return int(fn(*args)), []
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int] * len(args) + [ctypes.POINTER(LL), ctypes.c_int]
    buf = (LL * (3 * CAP))(*([FILL] * (3 * CAP)))
    ret = int(fn(*args, buf, cap))
    used = 3 * max(ret, 0)
    assert used <= 3 * CAP and all(v == FILL for v in buf[used:]), (name, args, cap, ret)
    return ret, [int(v) for v in buf[:used]]


def main(paths):
    libs = [ctypes.CDLL(p) for p in paths]
    records = []
    for name, args, cap in cases():
        got = [replay(lib, name, args, cap) for lib in libs]
        assert all(g == got[0] for g in got), ('the libraries disagree', name, args, cap)
        records.append({'fn': name, 'args': list(args), 'max': cap, 'ret': got[0][0], 'out': got[0][1]})
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, 'w') as f:
        f.write('[\n' + ',\n'.join(json.dumps(r, separators=(',', ':')) for r in records) + '\n]\n')
    print('%d records -> %s' % (len(records), OUT))


if __name__ == '__main__':
    main(sys.argv[1:] or [os.path.join(ROOT, 'nele_gan_amd', n) for n in ('libnele_hip.so', 'libnele_hip_ab.so')])
