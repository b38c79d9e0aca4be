"""The golden inputs of tests/golden/p56.npz rebuilt from their recipes (tests/golden/make_golden_p56.py: case_input)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'p56.npz')


def load():
    """-> (npz, [(name, float32 samples)] in the file's order).  No case is left out."""
    from nele_gan_amd import synth
    g = np.load(GOLDEN)
    cases = []
    for i, name in enumerate(g['names'].tolist()):
        kind = str(g['kinds'][i])
        if kind == 'pcm':
            x = (g['pcm_' + name].astype(np.float32) / np.float32(32768.0)).astype(np.float32)
        elif kind == 'zeros':
            x = np.zeros(int(g['length'][i]), dtype=np.float32)
        else:
            x = (synth.clean_utterance(int(g['index'][i]), int(g['length'][i])) * np.float32(g['scale'][i])).astype(np.float32)
        assert len(x) == int(g['n'][i])
        cases.append((name, x))
    return g, cases


def rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-300)
