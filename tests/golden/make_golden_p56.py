#!/usr/bin/env python
"""Generate tests/golden/p56.npz by IMPORTING the reference's asl_P56 (build container only; like make_golden.py only data is written).

    python tests/golden/make_golden_p56.py [--ref /root/reference]

Inputs: the two toy clean files as int16 PCM (x = s / 32768), and seeded recipes otherwise (synth.clean_utterance(index, length) times a
float32 scale; zeros) - the tests rebuild those from the recipe (tests/test_p56_cpu.py: case_input).  The reference is run on FLOAT64
copies of the float32 samples (its `x.T @ x` goes through BLAS in the input's dtype otherwise).  Its counters `a` and `sq` are locals it
does not return: they are read from its frame when it returns (sys.setprofile).  The three inputs on which it fails with `c0` unset
(digital silence; long-term level below the margin; no threshold reaching the margin) are recorded with the status the library
defines for them: the reference only raises UnboundLocalError there, so WHICH of the three statuses an input has is decided by the
restatement tests/p56_ref.py (whose counters and sum of squares are checked against the reference's on that input first).  `pauses` is a
constructed signal (pauses_signal below): bursts with pauses that put the hangover's boundary - 3200 samples after an exceedance counts,
3201 does not - on exact sample distances.

Per input the script records the bisection margin: the smallest | |diff| - tol | over every comparison bin_interp made (its 0.5 dB stop
makes its output jump where one flips), taken from the restatement tests/p56_ref.py after that has been checked against the reference
on the same input.  An input whose margin is below 1e-6 dB must be replaced HERE (the script stops), never skipped in a test.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

# name, kind, synth index, length, scale
CASES = [
    ('toy_train', 'pcm', 0, 0, 1.0),
    ('toy_test', 'pcm', 0, 0, 1.0),
    ('synth_16384', 'synth', 0, 16384, 1.0),
    ('synth_40000', 'synth', 3, 40000, 1.0),
    ('synth_63871', 'synth', 1, 63871, 1.0),
    ('synth_128000', 'synth', 2, 128000, 1.0),
    ('synth_quiet', 'synth', 4, 48000, 0.01),
    ('synth_loud', 'synth', 6, 48000, 8.0),
    ('silence', 'zeros', 0, 8000, 0.0),
    ('below_margin', 'synth', 7, 16000, 0.003),
    ('no_crossing', 'synth', 8, 16000, 200.0),
    ('pauses', 'pcm', 0, 0, 1.0),
]
PCM_FILES = {'toy_train': 'Train_Clean.wav', 'toy_test': 'Test_Clean.wav'}
PAUSE_THRESHOLDS = (9, 11)
PAUSE_GAPS = (3200, 3201, 3202, 3203)


def exceedance_gaps(q, c):
    """samples from one exceedance q >= c to the next, wherever they are not adjacent"""
    idx = np.flatnonzero(q >= c)
    d = np.diff(idx)
    return d[d > 1]


def pauses_signal():
    """Bursts of 0.1 (int16 PCM) separated by pauses of about 0.2 s, each pause tuned so that for threshold 9 or 11 the envelope's last
    exceedance before the pause and its first one after it are exactly 3200 .. 3203 samples apart: 3201 apart, the pause's last sample is
    at hangover distance 3200 and still counts; 3202 apart, one sample does not.  Every such pause is longer than a 2048-sample chunk of
    the kernel, so the last exceedance is always carried over chunk and segment boundaries.  Ends with a pause longer than the hangover."""
    import p56_ref
    burst = (3277 * np.where(np.arange(1500) % 2 == 0, 1, -1)).astype(np.int16)
    sig = np.zeros(700, dtype=np.int16)
    for j in PAUSE_THRESHOLDS:
        for want in PAUSE_GAPS:
            sig = np.concatenate([sig, burst])
            pause = 3000
            for _ in range(20):
                trial = np.concatenate([sig, np.zeros(pause, dtype=np.int16), burst, np.zeros(600, dtype=np.int16)])
                q = p56_ref.envelope(trial.astype(np.float32) / np.float32(32768.0))
                ex = np.flatnonzero(q >= p56_ref.THRESHOLDS[j])
                nxt = ex[ex >= len(sig) + pause]
                got = int(nxt[0] - ex[ex < len(sig) + pause][-1])
                if got == want:
                    break
                pause += want - got
            assert got == want, (j, want, got)
            sig = np.concatenate([sig, np.zeros(pause, dtype=np.int16)])
    sig = np.concatenate([sig, burst, np.zeros(4500, dtype=np.int16)])
    q = p56_ref.envelope(sig.astype(np.float32) / np.float32(32768.0))
    for j in PAUSE_THRESHOLDS:
        assert set(PAUSE_GAPS) <= set(exceedance_gaps(q, p56_ref.THRESHOLDS[j]).tolist()), j
    return sig


def case_input(kind, index, length, scale, pcm=None):
    """float32 samples of a case (the tests use the same function through the recipe stored in the file)"""
    from nele_gan_amd import synth
    if kind == 'pcm':
        return (pcm.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    if kind == 'zeros':
        return np.zeros(int(length), dtype=np.float32)
    return (synth.clean_utterance(int(index), int(length)) * np.float32(scale)).astype(np.float32)


def read_pcm16(path):
    import wave
    with wave.open(path, 'rb') as w:
        assert w.getnchannels() == 1 and w.getsampwidth() == 2 and w.getframerate() == 16000
        return np.frombuffer(w.readframes(w.getnframes()), dtype='<i2').copy()


def run_reference(asl_P56, x64):
    """-> (result triple or None where the reference fails on its unset c0, its counters `a` as it left them, its sq)"""
    grabbed = {}

    def prof(frame, event, arg):
        if event == 'return' and frame.f_code is asl_P56.__code__:
            grabbed['a'] = np.array(frame.f_locals['a'], dtype=np.int64)
            grabbed['sq'] = float(np.asarray(frame.f_locals['sq']).reshape(-1)[0])
    sys.setprofile(prof)
    try:
        try:
            res = asl_P56(x64, 16000, 16)
        except UnboundLocalError:
            res = None
    finally:
        sys.setprofile(None)
    return res, grabbed['a'], grabbed['sq']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', default='/root/reference')
    a = ap.parse_args()
    sys.path.insert(0, a.ref)
    from asl_P56 import asl_P56
    import p56_ref
    out = {'names': np.array([c[0] for c in CASES]), 'kinds': np.array([c[1] for c in CASES]),
           'index': np.array([c[2] for c in CASES], dtype=np.int64), 'length': np.array([c[3] for c in CASES], dtype=np.int64),
           'scale': np.array([c[4] for c in CASES], dtype=np.float64)}
    rows = {k: [] for k in ('counts', 'sq', 'asl_msq', 'actfact', 'c0', 'status', 'margin_db', 'delta_margin_db', 'n')}
    for name, kind, index, length, scale in CASES:
        pcm = None
        if kind == 'pcm':
            pcm = pauses_signal() if name == 'pauses' else read_pcm16(os.path.join(HERE, 'toy', PCM_FILES[name]))
            out['pcm_' + name] = pcm
        x = case_input(kind, index, length, scale, pcm)
        res, cnt, sq = run_reference(asl_P56, x.astype(np.float64))
        mine = p56_ref.level(x)
        if res is None:                                    # the reference failed on its unset c0: the status the library defines
            status, triple = mine['status'], (0.0, 0.0, 0.0)
            assert status in (p56_ref.SILENT, p56_ref.BELOW_MARGIN, p56_ref.NO_CROSSING), name
            counts = cnt + 2 if status == p56_ref.SILENT else cnt      # (silence leaves before `a += 2`, with -1 each)
        else:
            status, triple, counts = 0, tuple(float(np.asarray(v).reshape(-1)[0]) for v in res), cnt
            assert mine['status'] == 0, (name, mine['status'])
            assert mine['margin_db'] >= 1e-6 and mine['delta_margin_db'] >= 1e-6, \
                "%s: a comparison of the tail is within %g / %g dB of flipping - replace this input" % (name, mine['margin_db'], mine['delta_margin_db'])
            for k_, v_ in zip(('asl_msq', 'actfact', 'c0'), triple):
                assert abs(mine[k_] - v_) <= 1e-9 * abs(v_), (name, k_, mine[k_], v_)
        assert (mine['counts'] == counts).all(), (name, mine['counts'], counts)
        assert abs(mine['sq'] - sq) <= 1e-11 * max(sq, 1e-300), (name, mine['sq'], sq)
        for k_, v_ in (('counts', counts), ('sq', sq), ('asl_msq', triple[0]), ('actfact', triple[1]), ('c0', triple[2]), ('status', status),
                       ('margin_db', mine['margin_db']), ('delta_margin_db', mine['delta_margin_db']), ('n', len(x))):
            rows[k_].append(v_)
        print('%-14s n %6d status %d asl_msq %.6e actfact %.4f c0 %.4e margin %.3g dB counts %s' %
              (name, len(x), status, triple[0], triple[1], triple[2], mine['margin_db'], counts.tolist()))
    out['counts'] = np.stack(rows['counts']).astype(np.int64)
    for k_ in ('sq', 'asl_msq', 'actfact', 'c0', 'margin_db', 'delta_margin_db'):
        out[k_] = np.array(rows[k_], dtype=np.float64)
    out['status'] = np.array(rows['status'], dtype=np.int32)
    out['n'] = np.array(rows['n'], dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, 'p56.npz'), **out)
    print('p56.npz written (%d cases)' % len(CASES))


if __name__ == '__main__':
    main()
