"""Noise at a chosen SNR from a pool of noise recordings, mixed on the GPU (csrc/level.hip; DESIGN.md "Noise mixing at an active-level SNR").

The SNR is defined once, here: speech level = ITU-T P.56 active speech level (``level='asl'``, asl_P56.batch_asl_P56) or the long-term
mean square (``level='rms'``); noise level = mean square of the segment that is added.  What is drawn for an utterance - pool recording,
start offset, SNR - is a pure function of (seed, utterance key, epoch): not of the batch, its size, the position in it or the rank.
"""
import hashlib

import numpy as np
import torch

from . import _lib, synth
from . import asl_P56 as _p56
from ._lib import call, ptr, stream

ZERO_NOISE, ZERO_LEVEL, BAD_ROW = (_lib.CONSTS['NELE_MIX_' + _n] for _n in ('ZERO_NOISE', 'ZERO_LEVEL', 'BAD_ROW'))


def draw_words(seed, key, epoch, n=3):
    """n 64-bit words of the counter-based generator: BLAKE2b of (seed, key, epoch).  ``key``: a string, or anything whose repr() is stable."""
    h = hashlib.blake2b(repr((int(seed), key if isinstance(key, str) else repr(key), int(epoch))).encode('utf-8'), digest_size=8 * n).digest()
    return [int.from_bytes(h[8 * i:8 * i + 8], 'little') for i in range(n)]


class NoiseMixer:
    def __init__(self, pool, snrs_db=synth.SNRS_DB, level='asl', seed=0, device='cuda', resample=False):
        """pool: a list of wav paths (16 kHz; read once, kept on the device as [N][Ln] float32 rows with their lengths) or a tensor / array
        [N, Ln] (every row Ln samples) or a pair (rows [N, Ln], lengths [N]).  snrs_db: the SNRs drawn from.  level: 'asl' or 'rms'.
        resample=True: pool files at other rates are resampled to 16 kHz on the GPU (resample.py) before the rows and the pool hash are
        formed, so tag() describes what is mixed; the default raises on them."""
        if level not in ('asl', 'rms'):
            raise ValueError("NoiseMixer: level must be 'asl' or 'rms'")
        self.level, self.seed, self.device = level, int(seed), device
        self.snrs_db = tuple(float(s) for s in snrs_db)
        if not self.snrs_db:
            raise ValueError("NoiseMixer: no SNR to draw from")
        self.pool_names = None
        if isinstance(pool, (list, tuple)) and len(pool) and isinstance(pool[0], str):
            from . import dataio
            sig = []
            for p in pool:
                x, sr = dataio.load(p)
                if sr != 16000 and resample and len(x):
                    from .resample import resample_host
                    x = resample_host(x, sr, 16000, device=device)
                elif sr != 16000:
                    raise ValueError("NoiseMixer: %s has sample rate %d, expected 16000" % (p, sr))
                if len(x) == 0:
                    raise ValueError("NoiseMixer: %s is empty" % p)
                sig.append(x)
            rows = np.zeros((len(sig), max(len(x) for x in sig)), dtype=np.float32)
            for r, x in enumerate(sig):
                rows[r, :len(x)] = x
            lens = np.asarray([len(x) for x in sig], dtype=np.int32)
            self.pool_names = [p.split('/')[-1] for p in pool]
        else:
            if isinstance(pool, (list, tuple)):
                rows, lens = pool
            else:
                rows, lens = pool, None
            rows = rows.detach().cpu().numpy() if hasattr(rows, 'detach') else np.asarray(rows)
            rows = np.ascontiguousarray(rows, dtype=np.float32)
            if rows.ndim != 2 or rows.shape[0] == 0 or rows.shape[1] == 0:
                raise ValueError("NoiseMixer: pool must be [N, Ln]")
            lens = np.full(rows.shape[0], rows.shape[1], dtype=np.int32) if lens is None else np.asarray(
                lens.cpu() if hasattr(lens, 'cpu') else lens, dtype=np.int32)
            if lens.shape != (rows.shape[0],) or (lens < 1).any() or (lens > rows.shape[1]).any():
                raise ValueError("NoiseMixer: pool lengths must be [N], each in 1 .. Ln")
        self.pool_lengths_host = lens
        h = hashlib.blake2b(digest_size=8)                  # what the pool holds, for tag(): lengths and samples
        h.update(np.ascontiguousarray(lens, dtype='<i4').tobytes())
        for r in range(rows.shape[0]):
            h.update(np.ascontiguousarray(rows[r, :lens[r]]).tobytes())
        self.pool_hash = h.hexdigest()
        self.pool = torch.from_numpy(rows).to(device)
        self.pool_lengths = torch.from_numpy(lens).to(device)
        self._levels = {}                                   # level key (what identifies the clean SIGNAL) -> (speech level, level meter's status)
        self.last = None                                    # what the last mix() drew and measured (mix_corpus writes it down)

    def tag(self):
        """identifies what this mixer draws (for cache keys beside the epoch)"""
        return ('mix', self.seed, self.level, self.snrs_db, int(self.pool.shape[0]), self.pool_hash)

    def draw(self, keys, epoch, lengths=None):
        """-> (rows int32 [B], offsets int32 [B], snr_db float64 [B]) on the host, each a function of (seed, key, epoch) only.
        (``lengths`` is accepted for symmetry with mix(); the draw does not depend on it.)"""
        n = len(keys)
        rows, offs, snr = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.float64)
        for i, k in enumerate(keys):
            w = draw_words(self.seed, k, epoch)
            rows[i] = w[0] % len(self.pool_lengths_host)
            offs[i] = w[1] % int(self.pool_lengths_host[rows[i]])
            snr[i] = self.snrs_db[w[2] % len(self.snrs_db)]
        return rows, offs, snr

    def speech_level(self, clean, lengths, level_keys=None):
        """-> (float64 [B] on the device: asl_msq of each row, or sq / length for level='rms'; the level meter's status int32 [B] on the host
        or device; the meter's result dict or None).  ``level_keys`` [B]: one hashable per row that identifies the clean SIGNAL (its file's
        path - not a name two folders may share): levels of known keys come from the mixer's table (a clean-signal quantity, measured once
        per utterance), bit-identical to measuring again.  None: every row is measured."""
        dev = clean.device
        if level_keys is not None and all(k in self._levels for k in level_keys):
            known = [self._levels[k] for k in level_keys]
            lv = np.asarray([v[0] for v in known], dtype=np.float64)
            return torch.from_numpy(lv).to(dev), np.asarray([v[1] for v in known], dtype=np.int32), None
        r = _p56.batch_asl_P56(clean, lengths)
        if self.level == 'asl':
            lv = r['asl_msq']
        else:
            n = torch.full((clean.shape[0],), clean.shape[1], dtype=torch.float64, device=dev) if lengths is None else lengths.to(torch.float64)
            lv = torch.where(n > 0, r['sq'] / torch.clamp(n, min=1.0), torch.zeros_like(n))
        st = r['status']
        if level_keys is not None:
            st = st.cpu().numpy()
            for k, v, s_ in zip(level_keys, lv.cpu().tolist(), st.tolist()):
                self._levels[k] = (v, int(s_))
        return lv, st, r

    def mix(self, clean, lengths, keys, epoch, level_keys=None):
        """clean [B, L] float32 (device), lengths [B] (device int32 or None), keys [B] -> noise [B, L] float32: for each utterance its drawn
        pool segment (wrapping at the recording's end) scaled to the drawn SNR against the utterance's speech level; zeros behind each
        row's end, and a zero row where the speech level or the segment's energy is zero (``last['status']``; ``last['p56_status']`` says
        why a level is zero).  ``keys`` select what is DRAWN (with seed and epoch); ``level_keys`` (see speech_level) only let the mixer
        remember a signal's level - without them every call measures it."""
        from .audio_util import _dev, _i32
        clean = _dev(clean, self.device).float()
        B, L = clean.shape
        dev = clean.device
        lengths = _i32(lengths, dev)
        if len(keys) != B or (level_keys is not None and len(level_keys) != B):
            raise ValueError("NoiseMixer.mix: one key per row")
        rows, offs, snr = self.draw(keys, epoch)
        lv, p56_status, meter = self.speech_level(clean, lengths, level_keys)
        packed = torch.from_numpy(np.concatenate([rows, offs])).to(dev)
        d_snr = torch.from_numpy(snr).to(dev)
        noise = torch.empty((B, L), dtype=torch.float32, device=dev)
        gain = torch.empty((B,), dtype=torch.float64, device=dev)
        status = torch.empty((B,), dtype=torch.int32, device=dev)
        call('nele_mix_noise_var', ptr(self.pool), ptr(self.pool_lengths), int(self.pool.shape[0]), int(self.pool.shape[1]), ptr(packed[:B]),
             ptr(packed[B:]), ptr(d_snr), ptr(lv.contiguous()), ptr(lengths), B, L, ptr(noise), ptr(gain), ptr(status), stream())
        self.last = {'rows': rows, 'offsets': offs, 'snr_db': snr, 'level': lv, 'gain': gain, 'status': status, 'p56_status': p56_status, 'meter': meter}
        return noise
