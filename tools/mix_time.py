#!/usr/bin/env python
"""Device time of the level meter and the mixing kernel, and one training epoch on fresh mixes against the same epoch from noise files.

    python tools/mix_time.py [--out profiles/mixing/mix_time.json] [--no-epoch]

Kernels: nele_asl_p56_var and nele_mix_noise_var at 256 x 4 s and 128 x 8 s (HIP events around one launch, median of 20 after 3 warm-up
launches), beside the same batch's STFT + band features + IMCRA (audio_util.stft_band + noise_band) - the cost the level meter is to be
compared with.  Epoch: GanTrainer.run_epoch over 256 utterances of 3 - 4 s in batches of 64 from wav files on tmpfs (bench.py's
epoch_from_files corpus), fed (a) from prepared noise files and (b) by FileBatches with a NoiseMixer, in alternating order (a b a b a b),
medians reported.  The mixer's table of speech levels is warm in (b): the level meter is NOT in that figure; `first_mixer_epoch_ms` is
the one epoch of a fresh mixer that measures all 256 levels (its batches' plans warm).
Against another tree (the parent commit, built in its own folder): `--tree DIR --files-only --out A.json` runs (a) alone with DIR's
package - run it and this tree's `--files-only` as separate processes in alternating order and compare the medians."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = sys.argv[sys.argv.index('--tree') + 1] if '--tree' in sys.argv else ROOT
sys.path.insert(0, os.path.abspath(TREE))


def dev_ms(fn, reps=20, warm=3):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return {'median_ms': statistics.median(ts), 'min_ms': min(ts), 'max_ms': max(ts), 'reps': reps}


def kernels():
    import numpy as np
    import torch
    from nele_gan_amd import audio_util as au, synth
    from nele_gan_amd.asl_P56 import batch_asl_P56
    from nele_gan_amd.mixing import NoiseMixer
    out = {}
    base = np.stack([synth.clean_utterance(9000 + k, 128000) for k in range(8)])
    pool = np.stack([synth.noise_utterance(70 + k, 160000) for k in range(4)])
    for B, L in ((256, 64000), (128, 128000)):
        wav = torch.from_numpy(np.ascontiguousarray(base[np.arange(B) % 8, :L])).cuda()
        keys = ['u%d' % k for k in range(B)]
        mixer = NoiseMixer(pool, seed=1)
        mixer.mix(wav, None, keys, 0, level_keys=keys)     # (levels now in the mixer's table: mix() below times the mixing kernel's path alone)
        noise = mixer.mix(wav, None, keys, 1, level_keys=keys)
        r = {'asl_p56': dev_ms(lambda: batch_asl_P56(wav)), 'mix_noise (levels known)': dev_ms(lambda: mixer.mix(wav, None, keys, 1, level_keys=keys)),
             'mix_noise (levels measured)': dev_ms(lambda: mixer.mix(wav, None, keys, 1)),
             'stft_band (clean)': dev_ms(lambda: au.stft_band(wav)), 'noise_band (STFT + IMCRA)': dev_ms(lambda: au.noise_band(noise))}
        out['%d x %d' % (B, L)] = r
        print(B, L, {k: round(v['median_ms'], 3) for k, v in r.items()}, flush=True)
    return out


def epochs(n_utt=256, batch=64, pairs=3, files_only=False):
    import numpy as np
    import torch
    from nele_gan_amd import dataio, synth
    from nele_gan_amd.train_nele import GanTrainer
    if not files_only:
        from nele_gan_amd.mixing import NoiseMixer
    root = tempfile.mkdtemp(prefix='nele_mix_', dir='/dev/shm' if os.path.isdir('/dev/shm') else None)
    try:
        c, v = synth.batch(n_utt, 64000, start=40000)
        rs = np.random.RandomState(0)
        for sub in ('Clean', 'Noise', 'Pool'):
            os.makedirs(root + '/' + sub)
        files = []
        for i in range(n_utt):
            L = int(rs.randint(48000, 64001))
            dataio.write_wav_pcm16('%s/Clean/u%04d.wav' % (root, i), c[i, :L])
            dataio.write_wav_pcm16('%s/Noise/u%04d.wav' % (root, i), v[i, :L])
            files.append('%s/Clean/u%04d.wav' % (root, i))
        for i in range(8):
            dataio.write_wav_pcm16('%s/Pool/n%d.wav' % (root, i), synth.noise_utterance(500 + i, 160000))
        mixer = None if files_only else NoiseMixer(sorted(dataio.get_filepaths(root + '/Pool')), seed=0)
        tr = GanTrainer('siib&haspi&estoi')
        ffb = dataio.FileBatches(files, root + '/Noise/', batch=batch, ahead=2, keep=2)

        def one(ep, mixed):
            fb = dataio.FileBatches(files, None, batch=batch, ahead=2, keep=2, mixer=mixer, epoch=ep) if mixed else ffb
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.run_epoch(ep, fb, (), d_batch=batch, sample_dir=root + '/out')
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if mixed:
                fb.close()
            return dt
        ep = 2
        kinds = (False,) if files_only else (False, True)
        for mixed in kinds * 2:                            # warm-up: plans, buffer sets, the mixer's level table
            one(ep, mixed)
            ep += 1
        ts = {False: [], True: []}
        for _ in range(pairs):
            for mixed in kinds:
                ts[mixed].append(one(ep, mixed))
                ep += 1
        if files_only:
            ffb.close()
            out = {'tree': os.path.abspath(TREE), 'epoch_from_files_ms': ts[False], 'median_from_files_ms': statistics.median(ts[False])}
            print(out, flush=True)
            return out
        mixer = NoiseMixer(sorted(dataio.get_filepaths(root + '/Pool')), seed=0)      # a fresh mixer: every level measured in this epoch
        first = one(ep, True)
        ffb.close()
        out = {'utterances': n_utt, 'batch': batch, 'order': 'files, mixer alternating, %d pairs after 2 warm-up pairs' % pairs,
               'epoch_from_files_ms': ts[False], 'epoch_with_mixer_ms': ts[True],
               'median_from_files_ms': statistics.median(ts[False]), 'median_with_mixer_ms': statistics.median(ts[True]),
               'first_mixer_epoch_ms': first, 'note': 'epoch_with_mixer: speech levels known (level meter not included); first_mixer_epoch: all measured'}
        print(out, flush=True)
        return out
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mixing', 'mix_time.json'))
    ap.add_argument('--no-epoch', action='store_true')
    ap.add_argument('--tree', default=ROOT, help="repository root whose package is timed (default: this file's)")
    ap.add_argument('--files-only', action='store_true', help='only the epoch from prepared noise files (works on trees without the mixer)')
    a = ap.parse_args()
    if a.files_only:
        res = {'epoch': epochs(files_only=True)}
    else:
        res = {'kernels': kernels()}
        if not a.no_epoch:
            res['epoch'] = epochs()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
    print('wrote', a.out)
