#!/usr/bin/env python
"""Device time of nele_ssdrc (csrc/ssdrc.hip), per kernel and as a whole, at 256 x 4 s and 128 x 8 s.

    python tools/ssdrc_time.py [--out profiles/ssdrc/ssdrc_time.json]

Whole call: HIP events around one ssdrc() call, median of 20 after 3 warm-up calls (the workspace allocation comes from torch's caching
allocator: no hipMalloc inside the timed region after the warm-up).  Per kernel: the library's HIP-event hook (nele_profile_begin) around
each tagged launch of the same calls - `ssdrc_voicing` covers the table kernel and the voicing kernel - median over the calls, and each
kernel's share of their sum; the serial attack / release chain is `ssdrc_gain`."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TAGS = ('ssdrc_voicing', 'ssdrc_shape', 'ssdrc_ola', 'ssdrc_envelope', 'ssdrc_gain', 'ssdrc_final')


def main():
    import numpy as np
    import torch
    from nele_gan_amd import _lib, ssdrc, synth
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ssdrc', 'ssdrc_time.json'))
    ap.add_argument('--reps', type=int, default=20)
    a = ap.parse_args()
    base = np.stack([synth.clean_utterance(9000 + k, 128000) for k in range(8)])
    res = {'device': _lib.device_info(), 'reps': a.reps, 'shapes': {}}
    for B, L in ((256, 64000), (128, 128000)):
        wav = torch.from_numpy(np.ascontiguousarray(base[np.arange(B) % 8, :L])).cuda()
        for _ in range(3):
            ssdrc.ssdrc(wav)
        torch.cuda.synchronize()
        whole = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ssdrc.ssdrc(wav)
            e1.record()
            e1.synchronize()
            whole.append(e0.elapsed_time(e1))
        _lib.profile_begin(','.join(TAGS))
        for _ in range(a.reps):
            ssdrc.ssdrc(wav)
        torch.cuda.synchronize()
        per = {t: statistics.median(_lib.profile_collect_tag(t)) for t in TAGS}
        _lib.profile_begin(None)
        tot = sum(per.values())
        r = {'whole_call_median_ms': statistics.median(whole), 'whole_call_min_ms': min(whole), 'whole_call_max_ms': max(whole),
             'kernel_median_ms': per, 'kernel_share': {t: v / tot for t, v in per.items()}, 'kernel_sum_ms': tot,
             'workspace_MiB': int(_lib.lib.nele_ssdrc_ws_bytes(B, L)) / 2.0 ** 20, 'seconds_of_speech': B * L / 16000.0}
        res['shapes']['%d x %d' % (B, L)] = r
        print(B, L, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
