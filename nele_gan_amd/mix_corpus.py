"""``python -m nele_gan_amd.mix_corpus --clean DIR --noise-pool DIR --out ROOT``: the noise folder the training and evaluation paths
consume, made from speech recordings and noise recordings.  For every ``<name>.wav`` under --clean it writes ``ROOT/Noise/<name>.wav``
(PCM_16, as long as the clean file) - a segment of a pool recording scaled to an SNR against the file's active speech level
(mixing.NoiseMixer: what is drawn follows (seed, file name, epoch) alone) - and ``ROOT/mix_manifest.csv`` with one line per file:
name, pool file, offset, snr_db, asl_msq, actfact, status (mixing status NELE_MIX_*, 0 = mixed), p56_status (the level meter's NELE_P56_*:
why a speech level is zero), clipped_samples (samples beyond PCM_16's range, saturated in the file: the SNR of such a file is not the
one asked for).  With ``--multienh ssdrc`` the same pass also writes ``ROOT/MultiEnh/<name>.wav``, the SSDRC of the clean file (ssdrc.py), and
``ROOT/ssdrc_manifest.csv``."""
import os

import numpy as np

MANIFEST_COLUMNS = ('name', 'pool_file', 'offset', 'snr_db', 'asl_msq', 'actfact', 'status', 'p56_status', 'clipped_samples')


def mix_corpus(clean_files, mixer, out_root, epoch=0, batch=32, workers=8, device='cuda', multienh=None):
    """-> manifest rows.  ``clean_files``: paths; ``mixer``: mixing.NoiseMixer; ``multienh='ssdrc'``: MultiEnh/ in the same pass."""
    import csv
    from . import asl_P56, dataio
    if multienh not in (None, 'ssdrc'):
        raise ValueError("mix_corpus: multienh must be None or 'ssdrc'")
    noise_dir = os.path.join(out_root, 'Noise')
    dataio.creatdir(noise_dir)
    rows, enh_rows = [], []
    if multienh:
        from . import ssdrc as _ssdrc
        enh_dir = os.path.join(out_root, 'MultiEnh')
        dataio.creatdir(enh_dir)
    fb = dataio.FileBatches(list(clean_files), None, batch=batch, workers=workers, device=device, mixer=mixer, epoch=epoch)
    try:
        for b in fb:
            if multienh:
                enh_rows += _ssdrc.write_batch(enh_dir, b['names'], b['clean'], _ssdrc.ssdrc(b['clean'], b['lengths']), b['lengths_host'], workers)
            drawn = b['mix']
            meter = drawn['meter'] if drawn['meter'] is not None else asl_P56.batch_asl_P56(b['clean'], b['lengths'])
            noise = b['noise'].cpu().numpy()
            clipped = (np.abs(noise) * np.float32(32767.0) > 32767.5).sum(axis=1)       # samples PCM_16 cannot hold: saturated, and counted
            dataio.write_wav_batch_pcm16([os.path.join(noise_dir, nm) for nm in b['names']], np.ascontiguousarray(dataio.pcm16_quantise(noise)),
                                         b['lengths_host'], threads=workers)
            asl, act, st = meter['asl_msq'].cpu().numpy(), meter['actfact'].cpu().numpy(), drawn['status'].cpu().numpy()
            p56 = meter['status'].cpu().numpy()
            for k, nm in enumerate(b['names']):
                r = int(drawn['rows'][k])
                rows.append((nm, mixer.pool_names[r] if mixer.pool_names else str(r), int(drawn['offsets'][k]), '%g' % float(drawn['snr_db'][k]),
                             '%.17g' % float(asl[k]), '%.17g' % float(act[k]), int(st[k]), int(p56[k]), int(clipped[k])))
    finally:
        fb.close()
    with open(os.path.join(out_root, 'mix_manifest.csv'), 'w', newline='') as fh:
        w = csv.writer(fh, lineterminator='\n')          # (names with commas are quoted)
        w.writerow(MANIFEST_COLUMNS)
        w.writerows(rows)
    if multienh:
        _ssdrc.write_manifest(out_root, enh_rows)
    return rows


def main(argv=None):
    import argparse
    from . import dataio, mixing, synth
    ap = argparse.ArgumentParser(prog='python -m nele_gan_amd.mix_corpus', description=__doc__)
    ap.add_argument('--clean', required=True, help='folder of clean wav files (16 kHz)')
    ap.add_argument('--noise-pool', required=True, help='folder of noise recordings (16 kHz)')
    ap.add_argument('--out', required=True, help='corpus root: Noise/ and mix_manifest.csv are written under it')
    ap.add_argument('--snr', default=None, help='comma-separated SNRs in dB to draw from (default: -11,-9,-7,-5,-3,-1)')
    ap.add_argument('--snr-level', choices=('asl', 'rms'), default='asl')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--epoch', type=int, default=0, help='which of the per-epoch draws to write (0: what validation without noise files uses)')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--multienh', choices=('ssdrc',), default=None, help='also write MultiEnh/: the SSDRC of every clean file (ssdrc.py)')
    ap.add_argument('--resample', action='store_true', help='resample pool files that are not at 16 kHz on the GPU instead of stopping on them')
    a = ap.parse_args(argv)
    clean = sorted(dataio.get_filepaths(a.clean))
    pool = sorted(dataio.get_filepaths(a.noise_pool))
    if not clean or not pool:
        ap.error('no wav file under %s' % (a.clean if not clean else a.noise_pool))
    mixer = mixing.NoiseMixer(pool, snrs_db=[float(v) for v in a.snr.split(',')] if a.snr else synth.SNRS_DB, level=a.snr_level, seed=a.seed, resample=a.resample)
    rows = mix_corpus(clean, mixer, a.out, epoch=a.epoch, batch=a.batch, multienh=a.multienh)
    bad, clip = sum(1 for r in rows if r[6] != 0), sum(1 for r in rows if r[8] != 0)
    print('%d noise files under %s/Noise (%d not mixed: zero speech level or silent noise segment; %d with clipped samples - see mix_manifest.csv)'
          % (len(rows), a.out.rstrip('/'), bad, clip))
    return 0


if __name__ == '__main__':
    import sys
    sys.exit(main())
