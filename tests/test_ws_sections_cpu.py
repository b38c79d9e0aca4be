"""The workspace sizes and section lists of the metric kernels (host-only functions: no GPU), pinned value for value.

CleanStateCache copies exactly the byte ranges the *_clean_sections functions name in place of running phase 3, and the stage tests read
the workspaces through the *_sections functions: an offset, stride or size that moves unnoticed would give scores from stale bytes.
tests/golden/ws_sections.json holds what every function answered before the layouts were described once in csrc/ws_arena.h (written by
tools/gen_ws_sections.py); both libraries of a build must answer the same, integer for integer."""
import ctypes
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('gen_ws_sections', os.path.join(ROOT, 'tools', 'gen_ws_sections.py'))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(gen.OUT) as _f:
    GOLDEN = json.load(_f)


def test_the_fixture_holds_every_case():
    assert [(r['fn'], tuple(r['args']), r['max']) for r in GOLDEN] == gen.cases()
    good = [r for r in GOLDEN if r['max'] is not None and r['ret'] > 0]
    assert {r['fn']: r['ret'] for r in good} == {name: n for name, (_na, n) in gen.SECTIONS.items()}
    assert all(len(r['out']) == 3 * r['ret'] for r in good)
    # the argument errors: one section short; a rate above 24 kHz and a signal below HASPI's minimum for the four functions that take a rate
    assert sum(na == 3 for (na, _n) in gen.SECTIONS.values()) == 4
    assert sum(r['ret'] < 0 for r in GOLDEN) == len(gen.SECTIONS) + 2 * 4


@pytest.mark.parametrize('name', ['libnele_hip.so', 'libnele_hip_ab.so'])
def test_sizes_and_sections_equal_the_recorded_ones(name):
    lib = ctypes.CDLL(os.path.join(ROOT, 'nele_gan_amd', name))
    for r in GOLDEN:
        ret, out = gen.replay(lib, r['fn'], r['args'], r['max'])
        assert (ret, out) == (r['ret'], r['out']), (r['fn'], r['args'], r['max'])
