"""Reverberant listening conditions for a batch whose rows have their own room (reference eval_metrics.py:118-169; DESIGN "Rooms").

    RirBank(rirs, tau=32)      impulse responses by name, their direct-path truncations, and both as one prepared device bank
    Room(bank).apply(...)      per row what eval_metrics.listening_condition gives for that row's RIR and length
    fir_fft(x, bank, index)    scipy.signal.lfilter(h[index[b]], [1], x[b]) -> nele_fir_fft_var (partitioned FFT convolution)

The bank holds 2 R entries: entry r is RIR r, entry R + r its direct path rir[:argmax + tau] (eval_metrics.py:127-131) - the same
filter with fewer taps.  Row id -1 = no room: the 'NO_rev' branch (:118-122)."""
import hashlib
import os

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream

fs = 16000


def _bytes(name, *args):
    n = getattr(_lib.lib, name)(*args)
    if n < 0:
        _lib.check(-1, name)
    return int(n)


def _i32(t, device):
    if t is None or (isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.device == device and t.is_contiguous()):
        return t
    return torch.as_tensor(np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t), dtype=torch.int32).to(device).contiguous()


def rir_name_of(file_name):
    """The reference's corpus convention (intel.py:196): '<utterance>#<rir>#<...>.wav' names its RIR in the middle field."""
    parts = os.path.basename(str(file_name)).split('#')
    return parts[1] if len(parts) > 1 else None


class RirBank:
    def __init__(self, rirs, tau=32, resolver=None, device='cuda', resample=False):
        """rirs: dict name -> 1-D array, or a folder of 16 kHz wav files (name = file name without '.wav').  resolver(file_name) -> RIR
        name or None replaces the '#' convention of ``ids``.  resample=True: a folder's files at other rates are resampled to 16 kHz on
        the GPU (resample.py) with gain sr_in / sr_out - a sampled impulse response carries the sampling period, so this keeps the
        filter's gain; argmax and tau then work on the 16 kHz response.  The default raises on them."""
        if isinstance(rirs, (str, os.PathLike)):
            from . import dataio
            found = {}
            for f in sorted(os.listdir(rirs)):
                if f.lower().endswith('.wav'):
                    x, sr = dataio.read_wav(os.path.join(rirs, f))
                    if sr != fs and resample:
                        from .resample import resample_host
                        x = resample_host(x, sr, fs, gain=sr / float(fs), device=device)
                    elif sr != fs:
                        raise ValueError('%s: %d Hz, expected %d' % (f, sr, fs))
                    found[f[:-4]] = x
            rirs = found
        if not rirs:
            raise ValueError('RirBank: no impulse responses')
        self.tau = int(tau)
        self.resolver = resolver
        self.names = list(rirs)
        self.rirs = [np.asarray(rirs[n], dtype=np.float32).reshape(-1) for n in self.names]   # eval_metrics.py:126 (float32 like the loaded file)
        self.b = [int(np.argmax(h)) for h in self.rirs]                                         # :127
        self.direct = [h[:b + self.tau] for h, b in zip(self.rirs, self.b)]                      # :128-131 (the zeros behind it filter nothing)
        self._index = {n: i for i, n in enumerate(self.names)}
        self.device = torch.device(device)
        self._dev = None

    def __len__(self):
        return len(self.names)

    def sample_hash(self):
        """hex digest over names, tau and samples: what a checkpoint records of the room it was trained in"""
        h = hashlib.sha256(('tau=%d' % self.tau).encode())
        for n, r in zip(self.names, self.rirs):
            h.update(n.encode())
            h.update(np.ascontiguousarray(r).tobytes())
        return h.hexdigest()

    def record(self):
        return {'names': list(self.names), 'tau': self.tau, 'hash': self.sample_hash()}

    def ids(self, file_names):
        """bank row of each corpus file name (numpy int32 [n]); -1: names no RIR of this bank -> anechoic row"""
        out = []
        for f in file_names:
            n = self.resolver(f) if self.resolver is not None else rir_name_of(f)
            if n is not None and n.lower().endswith('.wav'):
                n = n[:-4]
            out.append(self._index.get(n, -1))
        return np.asarray(out, dtype=np.int32)

    def name_of(self, i):
        return None if i < 0 else self.names[int(i)]

    def prepared(self):
        """-> (bank, shifts): the device bank of the 2 R filters (prepared once) and b per RIR (int32 device [R])"""
        if self._dev is None:
            R = len(self.rirs)
            filt = self.rirs + self.direct
            Lh = max(len(h) for h in filt)
            host = np.zeros((2 * R, Lh), dtype=np.float64)
            for i, h in enumerate(filt):
                host[i, :len(h)] = h
            taps = np.asarray([len(h) for h in filt], dtype=np.int32)
            bank = torch.empty(_bytes('nele_rir_bank_bytes', 2 * R, Lh), dtype=torch.uint8, device=self.device)
            d_h, d_t = torch.from_numpy(host).to(self.device), torch.from_numpy(taps).to(self.device)
            call('nele_rir_bank_prepare', ptr(d_h), ptr(d_t), 2 * R, Lh, ptr(bank), stream())
            torch.cuda.current_stream(self.device).synchronize()         # d_h / d_t die here
            self._dev = (bank, torch.as_tensor(np.asarray(self.b, dtype=np.int32)).to(self.device))
        return self._dev


def prepare_bank(filters, device='cuda'):
    """A bare device bank of ``filters`` (list of 1-D arrays), entry i = filters[i]: the C ABI's nele_rir_bank_prepare."""
    Lh = max(len(h) for h in filters)
    host = np.zeros((len(filters), Lh), dtype=np.float64)
    for i, h in enumerate(filters):
        host[i, :len(h)] = np.asarray(h, dtype=np.float64)
    taps = torch.as_tensor(np.asarray([len(h) for h in filters], dtype=np.int32)).to(device)
    bank = torch.empty(_bytes('nele_rir_bank_bytes', len(filters), Lh), dtype=torch.uint8, device=device)
    d_h = torch.from_numpy(host).to(device)
    call('nele_rir_bank_prepare', ptr(d_h), ptr(taps), len(filters), Lh, ptr(bank), stream())
    torch.cuda.current_stream().synchronize()
    return bank


def fir_fft(x, bank, rir_index=None, lengths=None, workspace=None):
    """x [B, L] float32 device, bank from prepare_bank / RirBank.prepared -> float64 [B, L]: row b filtered with entry rir_index[b]
    (None: entry 0), exact zeros behind lengths[b]."""
    x = x.contiguous()
    B, L = x.shape
    y = torch.empty((B, L), dtype=torch.float64, device=x.device)
    need = _bytes('nele_fir_fft_workspace_bytes', B, L)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=x.device)
    lengths, rir_index = _i32(lengths, x.device), _i32(rir_index, x.device)      # (held until the call is enqueued)
    call('nele_fir_fft_var', ptr(x), B, L, ptr(lengths), ptr(bank), ptr(rir_index), ptr(y), ptr(workspace), stream())
    return y


def norm_clip_var(a, add=None, lengths=None, add_shift=None, out_shift=None, target_rms=0.0, keep64=False):
    """eval_metrics.norm_clip with per-row lengths and shifts (nele_norm_clip_var)."""
    a = a.contiguous()
    B, N = a.shape
    is64 = a.dtype == torch.float64
    if not is64:
        a = a.float()
    out = torch.empty((B, N), dtype=torch.float64 if keep64 else torch.float32, device=a.device)
    call('nele_norm_clip_var', ptr(a) if is64 else None, None if is64 else ptr(a), ptr(add), B, N, ptr(lengths), ptr(add_shift), ptr(out_shift),
         float(target_rms), None if keep64 else ptr(out), ptr(out) if keep64 else None, None, stream())
    return out


class Room:
    """The listener's room, applied to a batch: Room(bank).apply(clean, enh, noise, rir_ids)."""

    def __init__(self, bank):
        self.bank = bank

    def _filter(self, x, index, lengths):
        # (the spectra workspace comes from torch's caching allocator per call: it belongs to the stream that uses it)
        return fir_fft(x, self.bank.prepared()[0], index, lengths)

    def clean_side(self, clean, rir_ids, lengths):
        """-> (clean_a, lengths_a, shift): the direct-path clean signal of each row (scaled to rms 0.03, clipped, shifted by the row's b;
        id -1: the clean row itself) - the part of ``apply`` that depends on the clean signal and the RIR alone."""
        dev = clean.device
        _, bs = self.bank.prepared()
        R = len(self.bank)
        ids = _i32(rir_ids, dev)
        dry = ids < 0
        safe = torch.clamp(ids, min=0)
        shift = torch.where(dry, torch.zeros_like(ids), bs[safe.long()]).to(torch.int32)
        direct = norm_clip_var(self._filter(clean, torch.where(dry, ids, safe + R).to(torch.int32), lengths), lengths=lengths, out_shift=shift, target_rms=0.03)
        clean_a = torch.where(dry[:, None], clean, direct)
        lengths_a = torch.clamp(lengths - shift, min=0).to(torch.int32)
        return clean_a, lengths_a, shift

    def degraded_side(self, enh, noise, rir_ids, lengths, shift):
        """-> mixed: each row's enhanced signal through its RIR, scaled to 0.03, clipped, shifted, plus the shifted noise, clipped."""
        dev = enh.device
        ids = _i32(rir_ids, dev)
        dry = ids < 0
        reverb = norm_clip_var(self._filter(enh, ids, lengths), lengths=lengths, out_shift=shift, target_rms=0.03, keep64=True)
        reverb = torch.where(dry[:, None], enh.double(), reverb)
        la = torch.clamp(lengths - shift, min=0).to(torch.int32)
        return norm_clip_var(reverb, add=noise, lengths=la, add_shift=shift)

    def apply(self, clean, enh, noise, rir_ids, lengths=None, enh_rms=0.0):
        """clean, enh, noise [B, L] float32 (columns beyond the shortest of the three are dropped: eval_metrics.py:111-114), rir_ids [B]
        (bank rows, -1 = anechoic), lengths [B] (None: full rows) -> (clean_a [B, L], mixed [B, L], lengths_a [B]) float32 / int32:
        left-aligned rows of lengths_a = lengths - b samples, zeros behind them."""
        dev = clean.device
        n = min(clean.shape[1], enh.shape[1], noise.shape[1])
        clean, enh, noise = (t[:, :n].float().contiguous() for t in (clean, enh, noise))
        B = clean.shape[0]
        lengths = torch.full((B,), n, dtype=torch.int32, device=dev) if lengths is None else torch.clamp(_i32(lengths, dev), max=n)
        if enh_rms > 0:                                                              # eval_metrics.py:104
            live = torch.arange(n, device=dev)[None, :] < lengths[:, None]
            e64 = torch.where(live, enh.double(), torch.zeros((), dtype=torch.float64, device=dev))
            enh = (e64 / torch.sqrt((e64 * e64).sum(dim=1, keepdim=True) / lengths[:, None].double()) * enh_rms).float()
        clean_a, lengths_a, shift = self.clean_side(clean, rir_ids, lengths)
        return clean_a, self.degraded_side(enh, noise, rir_ids, lengths, shift), lengths_a
