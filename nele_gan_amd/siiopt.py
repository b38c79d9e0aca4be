"""A training-free, noise-adaptive enhancer: SII-optimal band gains (Taal, Jensen & Leijon, "On optimal linear
filtering of speech for near-end listening enhancement", IEEE SPL 2013).

Per frame the speech energy is redistributed over the 64 bands so that an approximated Speech Intelligibility Index is maximal at
unchanged total power: closed-form water-filling on the long-term speech band powers and IMCRA's noise band powers - the generator's
own two inputs - giving a mask in the generator's own range.  The arithmetic is in libnele_hip.so (csrc/siiopt.h; ``nele_siiopt_mask``
offline, ``nele_rt_rule_hop`` per hop); there is none in torch.

    rule = SiiOptRule()                                        # strength 0.5, lam 0.98, the default band importance
    enh = Enhancer(G=rule).enhance(clean_wav, noise_wav)       # the offline chain with the rule in the generator's place
    rt = RealtimeEnhancer(rule=rule, streams=256)              # the real-time chain: no checkpoint needed
    python -m nele_gan_amd.siiopt --clean <dir> --noise <dir> --out <corpus>/Train      # noise-dependent pre-enhanced examples
"""
import os

import numpy as np
import torch

from . import _lib
from .audio_util import gmtband
from ._lib import call, ptr, stream

NB = 64
LAMBDA = _lib.CONSTS5['NELE_SIIOPT_LAMBDA']
# one-third-octave band centres (Hz) and their importances (they sum to 1): the contract of the default gamma, whatever a standard says
CENTRES = (160, 200, 250, 315, 400, 500, 630, 800, 1000, 1250, 1600, 2000, 2500, 3150, 4000, 5000, 6300, 8000)
IMPORTANCE = (0.0083, 0.0095, 0.0150, 0.0289, 0.0440, 0.0578, 0.0653, 0.0711, 0.0818, 0.0844, 0.0882, 0.0898, 0.0868, 0.0844, 0.0771, 0.0527,
              0.0364, 0.0185)
MANIFEST_COLUMNS = ('name', 'samples', 'clean_rms', 'peak', 'clipped')


def band_importance():
    """The default gamma [64] float64: the one-third-octave importances as a density I_j / (0.2316 f_j) at the centres, interpolated
    linearly in log f at the band's frequency 31.25 * gmtband[i] (0 below 160 Hz, held above 8 kHz), times the band's width
    31.25 * (gmtband[min(i + 1, 63)] - gmtband[max(i - 1, 0)]) / 2, normalised to sum 1."""
    fc = np.asarray(CENTRES, dtype=np.float64)
    dens = np.asarray(IMPORTANCE, dtype=np.float64) / (0.2316 * fc)
    g = np.zeros(NB, dtype=np.float64)
    for i in range(NB):
        f = 31.25 * gmtband[i]
        width = 31.25 * (gmtband[min(i + 1, NB - 1)] - gmtband[max(i - 1, 0)]) / 2
        if f < fc[0]:
            d = 0.0
        elif f >= fc[-1]:
            d = dens[-1]
        else:
            d = float(np.interp(np.log(f), np.log(fc), dens))
        g[i] = d * width
    return g / g.sum()


class SiiOptRule(torch.nn.Module):
    """The rule as a parameter-free module in the generator's place: ``forward(clean_band, noise_band) -> mask`` ([B, T, 64] float32 each,
    the generator's layouts), so ``inference.Enhancer(G=SiiOptRule())`` runs ``enhance`` and ``enhance_stream`` with both norms, and
    ``realtime.RealtimeEnhancer(rule=SiiOptRule())`` the real-time chain.  strength in (0, 1]: the exponent on the optimal gain (1: the
    optimum of the approximated SII itself; 0.5 scores better on SIIB and ESTOI); lam in [0, 1): the forgetting factor
    of the long-term speech power; importance: gamma [64] >= 0 with a positive sum (None: ``band_importance()``).  No gradients."""

    def __init__(self, strength=0.5, lam=LAMBDA, importance=None):
        super().__init__()
        strength, lam = float(strength), float(lam)
        if not (0.0 < strength <= 1.0):
            raise ValueError("SiiOptRule: strength must be in (0, 1] (got %r)" % (strength,))
        if not (0.0 <= lam < 1.0):
            raise ValueError("SiiOptRule: lam must be in [0, 1) (got %r)" % (lam,))
        g = band_importance() if importance is None else np.asarray(importance, dtype=np.float64).reshape(-1)
        if g.shape[0] != NB or not np.all(np.isfinite(g)) or np.any(g < 0) or not g.sum() > 0:
            raise ValueError("SiiOptRule: importance must hold 64 finite values >= 0 with a positive sum")
        self.strength, self.lam = strength, lam
        self.importance = np.ascontiguousarray(g)
        self._gamma = {}                      # device -> gamma on it
        # what inference.Enhancer asks of a generator it was handed: there are no weight layouts to freeze and no activation buffers
        self.precision = 'f32'
        self.buffer_slot = 0
        self._weights_frozen = False

    def gamma(self, device):
        dev = _lib.norm_dev(device)
        if dev not in self._gamma:
            self._gamma[dev] = torch.from_numpy(self.importance).to(dev)
        return self._gamma[dev]

    def rt_args(self, device):
        """the arguments nele_rt_rule_hop / _finish take where nele_rt_hop / _finish take the precision"""
        return [ptr(self.gamma(device)), self.lam, self.strength]

    def freeze_weights(self, dev=None):
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(_lib.norm_dev(dev or 'cuda')))
        return ev

    def unfreeze_weights(self):
        pass

    @torch.no_grad()
    def forward(self, clean_band, noise_band):
        x, y = clean_band, noise_band
        if x.dim() != 3 or x.shape[2] != NB or y.shape != x.shape:
            raise ValueError("SiiOptRule.forward: clean_band and noise_band must both be [B, T, 64]")
        if not x.is_cuda:
            raise RuntimeError("nele_gan_amd: the rule runs on the GPU only (no CPU fallback)")
        B, T, _ = x.shape
        xs, ys = x.detach().contiguous().float(), y.detach().contiguous().float()
        mask = torch.empty((B, T, NB), dtype=torch.float32, device=x.device)
        if B * T:
            call('nele_siiopt_mask', ptr(xs), ptr(ys), ptr(self.gamma(x.device)), B, T, self.lam, self.strength, ptr(mask), stream())
        return mask


# ------------------------------------------------------------------------------------------------ a folder of pre-enhanced examples
def pre_enhance(clean, noise, lengths, rule=None, enhancer=None):
    """The rule's output for the clean and noise rows of a batch as a PCM_16 file of it reads back: float32 [B, L] (values k / 32768,
    256 * (lengths // 256) samples per row, zeros behind) and those lengths.  What ``siiopt_corpus`` writes and what
    ``fit(multienh='siiopt')`` makes for a batch."""
    from .inference import Enhancer
    e = enhancer if enhancer is not None else Enhancer(G=rule if rule is not None else SiiOptRule(), device=clean.device, norm='utterance')
    y = e.enhance(clean, noise, pcm16=True, lengths=lengths)
    out = torch.zeros_like(clean)
    out[:, :y.shape[1]] = y
    n = torch.full((clean.shape[0],), clean.shape[1], dtype=torch.int32, device=clean.device) if lengths is None else lengths.to(torch.int32)
    return out, (n // 256) * 256


def siiopt_corpus(clean_files, noise_path, out_root, rule=None, batch=32, workers=8, device='cuda'):
    """``out_root/MultiEnh/<name>.wav`` (PCM_16) for every clean file - the rule's output against the noise file of the same name under
    ``noise_path`` - and ``out_root/siiopt_manifest.csv`` -> manifest rows, as ``ssdrc.ssdrc_corpus`` does for SSDRC."""
    import csv
    from . import dataio
    from .inference import Enhancer
    out_dir = os.path.join(out_root, 'MultiEnh')
    dataio.creatdir(out_dir)
    e = Enhancer(G=rule if rule is not None else SiiOptRule(), device=device, norm='utterance')
    fb = dataio.FileBatches(list(clean_files), noise_path, batch=batch, workers=workers, device=e.device)
    rows = []
    try:
        for b in fb:
            y, n = pre_enhance(b['clean'], b['noise'], b['lengths'], enhancer=e)
            codes = torch.round(y * 32768.0).to(torch.int16).cpu().numpy()             # y holds k / 32768 exactly
            nh = n.cpu().numpy().astype(np.int32)
            names = [nm.split('/')[-1] for nm in b['names']]
            dataio.write_wav_batch_pcm16([os.path.join(out_dir, nm) for nm in names], np.ascontiguousarray(codes), nh, threads=workers)
            peak = torch.abs(y).amax(dim=1).cpu().numpy()
            sq = (b['clean'].double() ** 2).sum(dim=1).cpu().numpy()
            lh = np.maximum(np.asarray(b['lengths_host'], dtype=np.int64), 1)
            clipped = ((codes == 32767) | (codes == -32768)).sum(axis=1)
            rows += [(nm, int(nh[k]), '%.9g' % float(np.sqrt(sq[k] / lh[k])), '%.9g' % float(peak[k]), int(clipped[k])) for k, nm in enumerate(names)]
    finally:
        fb.close()
    with open(os.path.join(out_root, 'siiopt_manifest.csv'), 'w', newline='') as fh:
        w = csv.writer(fh, lineterminator='\n')
        w.writerow(MANIFEST_COLUMNS)
        w.writerows(rows)
    return rows


def main(argv=None):
    import argparse
    from . import dataio
    ap = argparse.ArgumentParser(prog='python -m nele_gan_amd.siiopt', description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--clean', required=True, help='folder of clean wav files (16 kHz)')
    ap.add_argument('--noise', required=True, help='folder with the noise file of the same name for every clean file')
    ap.add_argument('--out', required=True, help='corpus root: MultiEnh/ and siiopt_manifest.csv are written under it')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--strength', type=float, default=0.5, help='exponent on the optimal gain, in (0, 1]')
    ap.add_argument('--lam', type=float, default=LAMBDA, help='forgetting factor of the long-term speech power, in [0, 1)')
    a = ap.parse_args(argv)
    if a.batch < 1:
        ap.error('--batch must be positive')
    try:
        rule = SiiOptRule(a.strength, a.lam)
    except ValueError as e:
        ap.error(str(e))
    clean = sorted(dataio.get_filepaths(a.clean))
    if not clean:
        ap.error('no wav file under %s' % a.clean)
    rows = siiopt_corpus(clean, a.noise.rstrip('/') + '/', a.out, rule, batch=a.batch)
    print('%d pre-enhanced files under %s/MultiEnh (%d with clipped samples - see siiopt_manifest.csv)'
          % (len(rows), a.out.rstrip('/'), sum(1 for r in rows if r[4] != 0)))
    return 0


if __name__ == '__main__':
    import sys
    sys.exit(main())
