"""SSDRC - spectral shaping and dynamic range compression (Zorila, Kandia and Stylianou, Interspeech 2012) - of clean speech on the GPU
(csrc/ssdrc.hip; the algorithm is fixed by DESIGN.md section 11).  It is what the reference's authors made their ``Train/MultiEnh`` files
with (train_nele.py:53) and the ``ssdrc`` baseline of its eval_metrics.py:107-108; it does not depend on the noise.

    ssdrc(wav, lengths=None, params=None, pcm16=False) -> wav         device tensors [B, L] or [L]
    python -m nele_gan_amd.ssdrc --clean DIR --out ROOT               ROOT/MultiEnh/<name>.wav (PCM_16) and ROOT/ssdrc_manifest.csv

``pcm16=True`` returns what a PCM_16 file of the output holds once it is read back (rint(y * 32767) saturated, / 32768): the tensor
dataio.FileBatches yields for the file the command line writes, bit for bit - the on-the-fly route of ``train_nele --multienh ssdrc``.
"""
import ctypes
import dataclasses
import os

import numpy as np
import torch

from . import _lib
from ._lib import c_double, c_int, call, ptr, stream

MAX_KNOTS = _lib.CONSTS['NELE_SSDRC_MAX_KNOTS']
MANIFEST_COLUMNS = ('name', 'samples', 'input_rms', 'peak', 'clipped_samples')


class nele_ssdrc_params(ctypes.Structure):
    _fields_ = [('shape', c_int), ('compress', c_int), ('lifter_q', c_int), ('n_knots', c_int), ('beta', c_double), ('preemph', c_double),
                ('attack', c_double), ('release', c_double), ('e0_ratio', c_double), ('knot_in_db', c_double * MAX_KNOTS),
                ('knot_out_db', c_double * MAX_KNOTS)]


@dataclasses.dataclass(frozen=True)
class SsdrcParams:
    """The parameters of DESIGN.md section 11 with its defaults (nele_ssdrc_params of include/nele_hip.h)."""
    shape: bool = True                                     # stage 1
    compress: bool = True                                  # stage 2
    lifter_q: int = 20                                     # Q: the envelope keeps quefrencies 2 .. Q
    beta: float = 0.25                                     # formant sharpening
    preemph: float = 0.3                                   # g of the adaptive pre-emphasis
    attack: float = 1e-4                                   # a_a
    release: float = 0.15                                  # a_r
    e0_ratio: float = 0.3                                  # e0 = e0_ratio * max e
    knots: tuple = ((-100.0, -100.0), (-60.0, -45.0), (-30.0, -15.0), (0.0, 0.0))     # (input dB, output dB), ascending, at most 8

    def c_struct(self):
        if not 2 <= len(self.knots) <= MAX_KNOTS:
            raise ValueError("SsdrcParams: 2 .. %d knots" % MAX_KNOTS)
        p = nele_ssdrc_params()
        p.shape, p.compress, p.lifter_q, p.n_knots = int(bool(self.shape)), int(bool(self.compress)), int(self.lifter_q), len(self.knots)
        p.beta, p.preemph, p.attack, p.release, p.e0_ratio = (float(self.beta), float(self.preemph), float(self.attack), float(self.release),
                                                              float(self.e0_ratio))
        for j, (xi, yo) in enumerate(self.knots):
            p.knot_in_db[j], p.knot_out_db[j] = float(xi), float(yo)
        return p

    @classmethod
    def from_c(cls, p):
        return cls(bool(p.shape), bool(p.compress), int(p.lifter_q), p.beta, p.preemph, p.attack, p.release, p.e0_ratio,
                   tuple((p.knot_in_db[j], p.knot_out_db[j]) for j in range(p.n_knots)))


def library_defaults():
    """-> SsdrcParams as nele_ssdrc_params_default fills them (the C ABI's own copy of the defaults)."""
    p = nele_ssdrc_params()
    call('nele_ssdrc_params_default', ctypes.byref(p))
    return SsdrcParams.from_c(p)


def _prepare(wav, lengths, dtype):
    from .audio_util import _dev, _i32
    wav = _dev(wav).to(dtype)
    one = wav.dim() == 1
    if one:
        wav = wav.unsqueeze(0)
    if wav.dim() != 2 or wav.shape[0] == 0 or wav.shape[1] == 0:
        raise ValueError("ssdrc: wav must be [B, L] or [L], not empty")
    wav = wav.contiguous()
    B, L = wav.shape
    nb = int(_lib.lib.nele_ssdrc_ws_bytes(B, L))
    ws = torch.empty((nb,), dtype=torch.uint8, device=wav.device)
    return wav, _i32(lengths, wav.device), ws, one


def ssdrc_shape(wav, lengths=None, params=None):
    """Stage 1 alone (nele_ssdrc_shape): float32 [B, L] -> float64 [B, L], no energy scaling."""
    x, ln, ws, one = _prepare(wav, lengths, torch.float32)
    s = torch.empty(x.shape, dtype=torch.float64, device=x.device)
    p = (params or SsdrcParams()).c_struct()
    call('nele_ssdrc_shape', ptr(x), ptr(ln), x.shape[0], x.shape[1], ctypes.byref(p), ptr(s), ptr(ws), stream())
    return s[0] if one else s


def ssdrc_compress(s, lengths=None, params=None):
    """Stage 2 alone (nele_ssdrc_compress): float64 [B, L] -> (y float64 [B, L] before the energy scaling, the smoothed envelope e-hat)."""
    x, ln, ws, one = _prepare(s, lengths, torch.float64)
    y, eh = torch.empty_like(x), torch.empty_like(x)
    p = (params or SsdrcParams()).c_struct()
    call('nele_ssdrc_compress', ptr(x), ptr(ln), x.shape[0], x.shape[1], ctypes.byref(p), ptr(y), ptr(eh), ptr(ws), stream())
    return (y[0], eh[0]) if one else (y, eh)


def pcm16_codes(y):
    """float32 -> the PCM_16 sample values a file of it holds (dataio.pcm16_quantise on the device): rint(y * 32767), saturated; float32."""
    return torch.clamp(torch.round(y * 32767.0), -32768.0, 32767.0)


def ssdrc(wav, lengths=None, params=None, pcm16=False):
    """wav float32 [B, L] or [L] (device; a numpy array is uploaded), lengths [B] (None: L each) -> the SSDRC-processed signal, same shape,
    same energy per row, exact zeros behind each row's length.  A row's result does not depend on the batch it is in."""
    x, ln, ws, one = _prepare(wav, lengths, torch.float32)
    y = torch.empty_like(x)
    p = (params or SsdrcParams()).c_struct()
    call('nele_ssdrc', ptr(x), ptr(ln), x.shape[0], x.shape[1], ctypes.byref(p), ptr(y), ptr(ws), stream())
    if pcm16:
        y = pcm16_codes(y) * (1.0 / 32768.0)
    return y[0] if one else y


# ------------------------------------------------------------------------------------------------ a folder of pre-enhanced examples
class _NoNoise:
    """dataio.FileBatches reads noise files or asks a mixer; SSDRC needs neither: a mixer that adds nothing."""
    last = {}

    def tag(self):
        return ('none',)

    def mix(self, clean, lengths, keys, epoch, level_keys=None):
        return torch.zeros_like(clean)


def _batches(clean_files, batch, workers, device):
    """the clean files as padded device batches {'clean', 'lengths', 'lengths_host', 'names'}"""
    from . import dataio
    fb = dataio.FileBatches(list(clean_files), None, batch=batch, workers=workers, device=device, mixer=_NoNoise())
    try:
        for b in fb:
            yield b
    finally:
        fb.close()


def write_batch(out_dir, names, clean, y, lengths_host, workers=8):
    """One batch of processed rows ``y`` (float32 [B, L], before quantisation) as PCM_16 files ``out_dir/<name>`` of lengths_host samples
    -> manifest rows.  Samples PCM_16 cannot hold are saturated in the file and counted."""
    from . import dataio
    codes = pcm16_codes(y)
    clipped = (torch.abs(y) * 32767.0 > 32767.5).sum(dim=1).cpu().numpy()
    peak = torch.abs(y).amax(dim=1).cpu().numpy()
    n = np.asarray(lengths_host, dtype=np.int64)
    sq = (clean.double() ** 2).sum(dim=1).cpu().numpy()
    rms = np.sqrt(sq / np.maximum(n, 1))
    dataio.write_wav_batch_pcm16([os.path.join(out_dir, nm) for nm in names], np.ascontiguousarray(codes.to(torch.int16).cpu().numpy()),
                                 np.asarray(lengths_host, dtype=np.int32), threads=workers)
    return [(nm, int(n[k]), '%.9g' % float(rms[k]), '%.9g' % float(peak[k]), int(clipped[k])) for k, nm in enumerate(names)]


def write_manifest(out_root, rows):
    import csv
    with open(os.path.join(out_root, 'ssdrc_manifest.csv'), 'w', newline='') as fh:
        w = csv.writer(fh, lineterminator='\n')              # (names with commas are quoted)
        w.writerow(MANIFEST_COLUMNS)
        w.writerows(rows)


def ssdrc_corpus(clean_files, out_root, params=None, batch=32, workers=8, device='cuda'):
    """``out_root/MultiEnh/<name>.wav`` for every clean file and ``out_root/ssdrc_manifest.csv`` -> manifest rows."""
    from . import dataio
    out_dir = os.path.join(out_root, 'MultiEnh')
    dataio.creatdir(out_dir)
    rows = []
    for b in _batches(clean_files, batch, workers, device):
        rows += write_batch(out_dir, b['names'], b['clean'], ssdrc(b['clean'], b['lengths'], params), b['lengths_host'], workers)
    write_manifest(out_root, rows)
    return rows


def main(argv=None):
    import argparse
    from . import dataio
    ap = argparse.ArgumentParser(prog='python -m nele_gan_amd.ssdrc', description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--clean', required=True, help='folder of clean wav files (16 kHz)')
    ap.add_argument('--out', required=True, help='corpus root: MultiEnh/ and ssdrc_manifest.csv are written under it')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--no-shape', action='store_true', help='switch the spectral shaping stage off')
    ap.add_argument('--no-compress', action='store_true', help='switch the dynamic range compression stage off')
    a = ap.parse_args(argv)
    if a.batch < 1:
        ap.error('--batch must be positive')
    clean = sorted(dataio.get_filepaths(a.clean))
    if not clean:
        ap.error('no wav file under %s' % a.clean)
    rows = ssdrc_corpus(clean, a.out, SsdrcParams(shape=not a.no_shape, compress=not a.no_compress), batch=a.batch)
    print('%d pre-enhanced files under %s/MultiEnh (%d with clipped samples - see ssdrc_manifest.csv)'
          % (len(rows), a.out.rstrip('/'), sum(1 for r in rows if r[4] != 0)))
    return 0


if __name__ == '__main__':
    import sys
    sys.exit(main())
