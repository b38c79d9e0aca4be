"""Active speech level (ITU-T P.56 method B): the host-side mirror of the reference's ``asl_P56.py``.

``asl_P56(x, fs, nbits)`` keeps the reference's name, argument order and return triple ``(asl_msq, actfact, c0)`` for one signal;
``batch_asl_P56`` takes a padded batch on the device.  The arithmetic runs in libnele_hip.so (csrc/level.hip, nele_asl_p56_var): the
reference's two-pass envelope in float64 in sample order, its 15 activity counters in their windowed form, its tolerance bisection.
Where the reference fails by accident (``c0`` unset: no active sample, a level below the margin, no threshold reaching the margin) the
library reports a status; ``asl_P56`` raises ValueError naming it, ``batch_asl_P56`` returns it with zeros.
"""
import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream

SILENT, BELOW_MARGIN, NO_CROSSING = (_lib.CONSTS['NELE_P56_' + _n] for _n in ('SILENT', 'BELOW_MARGIN', 'NO_CROSSING'))
STATUS_NAMES = {SILENT: 'NELE_P56_SILENT (no sample reaches the lowest threshold)',
                BELOW_MARGIN: 'NELE_P56_BELOW_MARGIN (long-term level less than 15.9 dB above the lowest threshold)',
                NO_CROSSING: 'NELE_P56_NO_CROSSING (no threshold reaches the 15.9 dB margin)'}
N_THRESHOLDS = 15


def batch_asl_P56(wav, lengths=None):
    """wav [B, L] float32 (device; a numpy array is uploaded), lengths [B] samples of each row (None: L) -> dict of device tensors:
    'asl_msq', 'actfact', 'c0', 'sq' float64 [B]; 'counts' int64 [B, 15] (the reference's counters after its ``a += 2``); 'status' int32 [B]
    (0, SILENT, BELOW_MARGIN or NO_CROSSING - the level values are zeros where it is not 0).  A row's results do not depend on the batch."""
    from .audio_util import _dev, _i32
    wav = _dev(wav).float()
    if wav.dim() != 2:
        raise ValueError("batch_asl_P56: wav must be [B, L]")
    B, L = wav.shape
    dev = wav.device
    out = {k: torch.empty((B,), dtype=torch.float64, device=dev) for k in ('asl_msq', 'actfact', 'c0', 'sq')}
    out['counts'] = torch.empty((B, N_THRESHOLDS), dtype=torch.int64, device=dev)
    out['status'] = torch.empty((B,), dtype=torch.int32, device=dev)
    nb = int(_lib.lib.nele_asl_p56_workspace_bytes(B, L))
    ws = torch.empty((nb,), dtype=torch.uint8, device=dev) if nb > 0 else None
    call('nele_asl_p56_var', ptr(wav), ptr(_i32(lengths, dev)), B, L, ptr(ws), nb, ptr(out['asl_msq']), ptr(out['actfact']), ptr(out['c0']),
         ptr(out['sq']), ptr(out['counts']), ptr(out['status']), stream())
    return out


def asl_P56(x, fs, nbits):
    """asl_P56.py:23 for one signal -> (asl_msq, actfact, c0) as Python floats.  fs = 16000 and nbits = 16 only (what the library builds)."""
    if int(fs) != 16000 or int(nbits) != 16:
        raise ValueError("asl_P56: fs = 16000 and nbits = 16 only (got fs = %r, nbits = %r)" % (fs, nbits))
    if hasattr(x, 'detach'):
        x = x.detach().cpu().numpy()
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(1, -1))
    if x.shape[1] == 0:
        raise ValueError("asl_P56: empty signal")
    r = batch_asl_P56(x)
    st = int(r['status'][0])
    if st != 0:
        raise ValueError("asl_P56: " + STATUS_NAMES.get(st, 'status %d' % st))
    return float(r['asl_msq'][0]), float(r['actfact'][0]), float(r['c0'][0])
