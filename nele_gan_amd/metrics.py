"""Batched objective metrics on the GPU: host-side mirror of the reference ``intel.py`` wrappers and
the ``read_batch_*`` fan-out of ``audio_util.py:120-203`` (there: 32 joblib processes over wav files;
here: one batched launch over utterances resident in HBM).

    ESTOI_Wrapper[_raw]_harvard(x, y, fs)   intel.py:122-134
    SIIB_Wrapper[_raw]_harvard(x, y, fs)    intel.py:57-100
    HASPI_Wrapper[_raw]_harvard(x, y, fs)   intel.py:108-114
    batch_estoi / batch_siib / batch_haspi (clean[B,L], degraded[B,L]) -> (raw[B], mapped[B])
    batch_hasqi / HasqiSplit (reference[B,L], processed[B,L]) -> float64 [B,7]: hasqi_v2 (pyhaspi2.py:32-74) as a training target

x is the clean reference, y the degraded signal (enhanced + noise, audio_util.py:139-141).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import c_int, c_longlong, call, ptr, stream

_ws_cache = {}


def _workspace(kind, nbytes, dev, cache=None):
    """Grow-only scratch buffer per (kind, device).  ``cache``: the dict that owns it - the module-global one for the one-shot batch_*
    calls, or a dict held by the caller (a GanTrainer) for the split objects' multi-GB workspaces, so that they are released with
    their owner instead of living until the process exits."""
    cache = _ws_cache if cache is None else cache
    key = (kind, str(dev))
    t = cache.get(key)
    if t is None or t.numel() < nbytes:
        t = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
        cache[key] = t
    return t


def release_workspaces():
    """Drop the module-global scratch buffers (they are re-created on demand)."""
    _ws_cache.clear()


class CleanStateCache:
    """Per-utterance clean-signal state of the split metrics, kept across calls (GanTrainer.enable_clean_cache).

    The reference scores the same <= 720 clean training files in every one of its 500 GAN epochs (train_nele.py:35-38,119,318-340) and
    recomputes the clean file's half of every metric each time.  That half is a pure function of the clean waveform: SIIB's VAD,
    clean spectra, covariance and KLT eigen-decomposition (phase 3 of nele_metric_siib_var: the step's single most expensive
    kernel chain), HASPI's whole reference-signal chain (phase 3 of nele_metric_haspi_var).  The library says which byte ranges of a
    workspace make up that state (nele_metric_{siib,haspi}_clean_sections); this class copies them out after phase 3 - one row per
    utterance and section in pooled device buffers - and copies them back in place of phase 3 when the same utterances come by again,
    at whatever rows of whatever batch.  Copies only: the scores are bit-identical to recomputation (tests/test_clean_cache_gpu.py).
    Keys: (kind, geometry = padded length L (+ fs, dither mode for HASPI), utterance key); the utterance key (file name, corpus id)
    stands for the clean waveform including its own length.  Never invalidated (clean files are immutable); once ``budget_bytes`` of device memory are in use, new utterances are simply not stored (they are recomputed)."""

    BLOCK_ROWS = 64

    def __init__(self, budget_bytes):
        self.budget = int(budget_bytes)
        self.used = 0
        self.pools = {}             # (kind, geometry) -> pool dict
        self.hits = self.misses = self.stored = self.declined = self.partial = 0
        self.poison = False         # tests: fill the workspace with 0xFF bytes before a restore (a forgotten section cannot go unnoticed)

    # kind -> (section list of the library, whether it takes the sampling rate)
    _SECTION_FUNCS = {'siib': ('nele_metric_siib_clean_sections', False), 'haspi': ('nele_metric_haspi_clean_sections', True),
                      'hasqi': ('nele_metric_hasqi_clean_sections', True)}

    @classmethod
    def _sections(cls, kind, B, L, fs):
        name, takes_fs = cls._SECTION_FUNCS[kind]
        buf = (c_longlong * (3 * 24))()
        n = getattr(_lib.lib, name)(int(B), int(L), *([int(fs)] if takes_fs else []), buf, 24)
        if n < 0:
            return None
        return [(int(buf[3 * k]), int(buf[3 * k + 1]), int(buf[3 * k + 2])) for k in range(n)]

    def _pool(self, kind, geom, L, fs):
        key = (kind, geom)
        p = self.pools.get(key)
        if p is None:
            sec = self._sections(kind, 1, L, fs)
            if sec is None:
                return None
            p = self.pools[key] = {'row_bytes': [b for (_o, st, b) in sec if st > 0], 'shared': None, 'blocks': [], 'index': {}, 'free': 0,
                                   'event': None, 'per_utt': sum(b for (_o, st, b) in sec if st > 0)}
        return p

    def lookup(self, kind, geom, keys, count=True):
        """-> list of (block, row) slots when EVERY utterance of the batch is cached, else None."""
        p = self.pools.get((kind, geom))
        if p is None or p['shared'] is None:
            self.misses += int(count)
            return None
        idx = p['index']
        slots = [idx.get(k) for k in keys]
        if any(s is None for s in slots):
            self.misses += int(count)
            return None
        self.hits += int(count)
        return slots

    def missing(self, kind, geom, keys):
        """Rows of the batch whose utterances are not cached yet, or None when the batch is better computed as a whole (nothing of it is
        cached, or the pool of this geometry does not exist yet)."""
        p = self.pools.get((kind, geom))
        if p is None or p['shared'] is None:
            return None
        rows = [i for i, k in enumerate(keys) if k not in p['index']]
        return rows if 0 < len(rows) < len(keys) else None

    @staticmethod
    def _runs(slots, rows=None):
        """[(block, row)] of batch rows ``rows`` (default: 0, 1, ..) -> runs (first batch row, block, first block row, count) of consecutive
        batch rows that sit in consecutive rows of one block"""
        rows = range(len(slots)) if rows is None else rows
        runs, k = [], 0
        while k < len(slots):
            b, r = slots[k]
            n = 1
            while k + n < len(slots) and rows[k + n] == rows[k] + n and slots[k + n] == (b, r + n):
                n += 1
            runs.append((rows[k], b, r, n))
            k += n
        return runs

    def restore(self, kind, geom, ws, B, L, fs, slots):
        """Copy the cached state of the batch's utterances into workspace ``ws`` (uint8 tensor) on the current stream."""
        p = self.pools[(kind, geom)]
        sec = self._sections(kind, B, L, fs)
        cur = torch.cuda.current_stream(ws.device)
        if p['event'] is not None:
            cur.wait_event(p['event'])           # the stores may have run on another stream
        if self.poison:
            ws.fill_(255)
        runs = self._runs(slots)
        j = sh = 0
        for (off, st, nb) in sec:
            if st == 0:
                ws[off:off + nb].copy_(p['shared'][sh])
                sh += 1
                continue
            view = ws[off:off + B * st].view(B, st)[:, :nb]
            for (k0, blk, r0, n) in runs:
                view[k0:k0 + n].copy_(p['blocks'][blk][j][r0:r0 + n])
            j += 1

    def store(self, kind, geom, ws, B, L, fs, keys):
        """Copy the state phase 3 just left in ``ws`` into the pool for the utterances not cached yet (current stream)."""
        p = self._pool(kind, geom, L, fs)
        if p is None:
            return False
        sec = self._sections(kind, B, L, fs)
        if p['shared'] is None:
            p['shared'] = [ws[off:off + nb].clone() for (off, st, nb) in sec if st == 0]
            self.used += sum(t.numel() for t in p['shared'])
        new = [(k, key) for k, key in enumerate(keys) if key not in p['index']]
        if not new:
            return True
        n_new = len(new)
        slots = []
        for _k, _key in new:
            if p['free'] == 0:
                need = self.BLOCK_ROWS * p['per_utt']
                if self.used + need > self.budget:
                    self.declined += len(new) - len(slots)
                    break
                p['blocks'].append([torch.empty((self.BLOCK_ROWS, nb), dtype=torch.uint8, device=ws.device) for nb in p['row_bytes']])
                p['free'] = self.BLOCK_ROWS
                self.used += need
            slots.append((len(p['blocks']) - 1, self.BLOCK_ROWS - p['free']))
            p['free'] -= 1
        new = new[:len(slots)]
        if not new:
            return False
        runs = self._runs(slots, [k for k, _key in new])
        j = 0
        for (off, st, nb) in sec:
            if st == 0:
                continue
            view = ws[off:off + B * st].view(B, st)[:, :nb]
            for (k0, blk, r0, n) in runs:
                p['blocks'][blk][j][r0:r0 + n].copy_(view[k0:k0 + n])
            j += 1
        for (_k, key), slot in zip(new, slots):
            p['index'][key] = slot
        self.stored += len(new)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(ws.device))
        p['event'] = ev
        return len(new) == n_new

    def stats(self):
        return {'hits': self.hits, 'misses': self.misses, 'partial': self.partial, 'stored': self.stored, 'declined': self.declined, 'bytes': self.used,
                'utterances': {'%s@%s' % k: len(p['index']) for k, p in self.pools.items()}}


def eigh_batched(A, return_repaired=False):
    """A [B,n,n] float64 symmetric (device) -> (eigenvalues [B,n] ascending, U [B,n,n] with rows = eigenvectors).
    return_repaired: also the number of matrices the cluster tridiagonalisation gave up on and the repair kernel redid (synchronises)."""
    A = A.clone().contiguous()
    B, n, _ = A.shape
    lam = torch.empty((B, n), dtype=torch.float64, device=A.device)
    U = torch.empty_like(A)
    ws = _workspace('eigh', _lib.lib.nele_eigh_workspace_bytes(B, n), A.device)
    call('nele_eigh_sym_batched', ptr(A), n, B, ptr(lam), ptr(U), ptr(ws), ws.numel(), stream())
    if return_repaired:
        return lam, U, int(_lib.lib.nele_eigh_repaired(ptr(ws), B, n))
    return lam, U


def eigh_batched_range(A, rel_cut, poison=False):
    """eigh_batched with eigenvectors on request (nele_eigh_sym_batched_range): -> (eigenvalues [B,n], U [B,n,n], kept_first [B] int32).
    Rows of U below 64 * (kept_first // 64) are zero.  poison: U and kept_first start as NaN / -1 (tests: what is not written shows)."""
    A = A.clone().contiguous()
    B, n, _ = A.shape
    lam = torch.empty((B, n), dtype=torch.float64, device=A.device)
    U = torch.full_like(A, float('nan')) if poison else torch.empty_like(A)
    kf = torch.full((B,), -1, dtype=torch.int32, device=A.device)
    ws = _workspace('eigh', _lib.lib.nele_eigh_workspace_bytes(B, n), A.device)
    call('nele_eigh_sym_batched_range', ptr(A), n, B, ptr(lam), ptr(U), ptr(ws), ws.numel(), stream(), float(rel_cut), ptr(kf))
    return lam, U, kf


def siib_kept_first(ws, B, L):
    """Per utterance, the first KLT component the eigensolver computed in the last SIIB call (phase 0 / 2 / 3) on workspace ``ws``
    (numpy int32 [B]; synchronises)."""
    out = (c_int * int(B))()
    call('nele_metric_siib_kept_first', int(B), int(L), ptr(ws), out)
    return np.frombuffer(out, dtype=np.int32).copy()


def _pair(x, y):
    def dev(a):
        if isinstance(a, np.ndarray):
            a = torch.from_numpy(np.ascontiguousarray(a))
        if not a.is_cuda:
            a = a.cuda()
        return a.float()
    x, y = dev(x), dev(y)
    single = x.dim() == 1
    if single:
        x, y = x.unsqueeze(0), y.unsqueeze(0)
    L = min(x.shape[1], y.shape[1])                    # intel.py:58-60 (minL truncation)
    return x[:, :L].contiguous(), y[:, :L].contiguous(), single


def _lens(lengths, device):
    return None if lengths is None else torch.as_tensor(lengths).to(device=device, dtype=torch.int32).contiguous()


def batch_estoi(x, y, lengths=None):
    """clean x [B,L], degraded y [B,L] (16 kHz) -> (raw [B], mapped [B]) float32 device tensors.
    lengths [B]: samples of each utterance inside the padded batch (one launch for files of different lengths)."""
    x, y, _ = _pair(x, y)
    B, L = x.shape
    nb = _lib.lib.nele_metric_estoi_workspace_bytes(B, L)
    ws = _workspace('estoi', nb, x.device)
    raw = torch.empty(B, device=x.device)
    mapped = torch.empty(B, device=x.device)
    call('nele_metric_estoi_var', ptr(x), ptr(y), ptr(_lens(lengths, x.device)), B, L, ptr(ws), ws.numel(), ptr(raw), ptr(mapped), stream())
    return raw, mapped


def _section_rows(ws, sections, B):
    """Per-utterance sections {offset, stride, bytes} of workspace ``ws`` -> one numpy uint8 array [B, bytes] each (synchronises)."""
    return [ws[off:off + B * st].view(B, st)[:, :nb].cpu().numpy() for (off, st, nb) in sections]


def estoi_stages(x, y, lengths=None):
    """Diagnostic: batch_estoi on a workspace of its own (every byte 0xFF before the call: what a kernel does not write reads as NaN / -1)
    -> (raw float32 numpy [B], stages), the workspace read through nele_metric_estoi_sections.  stages[name][b] is row b's array, cut to the
    row's own sizes (n10 = ceil(5 len / 8) samples at 10 kHz, F frames of 256 at hop 128, nkept frames inside the 40 dB gate):
      'xr' [2, n10] x then y at 10 kHz; 'en' [F] dB; 'keep' [nkept] original frame of each kept frame; 'nkept' int;
      'tob' [2, 15, nkept] third-octave magnitudes of the silence-removed x then y; 'dseg' [max(nkept - 29, 0)] per-segment mean products."""
    x, y, _ = _pair(x, y)
    B, L = x.shape
    ws = torch.full((int(_lib.lib.nele_metric_estoi_workspace_bytes(B, L)),), 255, dtype=torch.uint8, device=x.device)
    raw = torch.empty(B, device=x.device)
    call('nele_metric_estoi_var', ptr(x), ptr(y), ptr(_lens(lengths, x.device)), B, L, ptr(ws), ws.numel(), ptr(raw), None, stream())
    buf = (c_longlong * 18)()
    n = _lib.lib.nele_metric_estoi_sections(B, L, buf, 6)
    if n != 6:
        _lib.check(n, 'nele_metric_estoi_sections')
    xr, en, keep, nkept, tob, dseg = _section_rows(ws, [(int(buf[3 * k]), int(buf[3 * k + 1]), int(buf[3 * k + 2])) for k in range(6)], B)
    lens = np.full(B, L) if lengths is None else np.minimum(np.asarray(torch.as_tensor(lengths).cpu()), L)
    nkept = nkept.view(np.int32)[:, 0].copy()
    out = {k: [] for k in ('xr', 'en', 'keep', 'tob', 'dseg')}
    out['nkept'] = nkept
    for b in range(B):
        n10 = -(-5 * int(lens[b]) // 8)
        F = (n10 - 256) // 128 + 1 if n10 >= 256 else 0
        nk = int(nkept[b])
        out['xr'].append(xr[b].view(np.float64).reshape(2, -1)[:, :n10].copy())
        out['en'].append(en[b].view(np.float64)[:F].copy())
        out['keep'].append(keep[b].view(np.int32)[:max(nk, 0)].copy())
        out['tob'].append(tob[b].view(np.float64).reshape(2, 15, -1)[:, :, :max(nk, 0)].copy())
        out['dseg'].append(dseg[b].view(np.float64)[:max(nk - 29, 0)].copy())
    return raw.cpu().numpy(), out


def siib_clean_stages(x, lengths=None):
    """Diagnostic: phase 3 of nele_metric_siib_var (the clean-signal half) on a workspace of its own (every byte 0xFF before the call)
    -> dict of per-row numpy arrays, read through nele_metric_siib_clean_sections.  What the buffers hold after phase 3 (csrc/siib.hip):
      'info' [B, 4] int = (M, frames of the M-times tiled signal, active frames na, status).  M is the replication factor of intel.py:93-97
          CLAMPED to 40 (status bit 1 set when the rule asked for more): every other buffer describes the signal tiled M <= 40 times.
      'xdb'[b] [info[b, 1]] float64: 10 log10(mean(frame^2) + eps) of EVERY frame f of the tiled signal, in the tiled frame numbering:
          frame f holds samples (200 f + j) mod len, j < 400, of the row (zero past M * len); nothing is materialised.
      'list'[b] [na] int: the active frames (xdb > order statistic - 40), ascending, in that tiled frame numbering.
      'XL'[b] [28, na] float64: band-major (row j = gammatone band j, column a = a-th ACTIVE frame): log band energies of the clean
          signal AFTER forward masking and BEFORE mean removal (the row mean is subtracted on the fly by the kernels that consume XL).
      'rowstat'[b] [28, 2] float64 of the clean signal: (band minimum BEFORE masking, band mean AFTER masking).
      'lam'[b] [420] float64: eigenvalues of the KLT covariance, ascending (all of them; eigenvectors exist above the 1e-10 cut only)."""
    sp = SiibSplit(x if torch.is_tensor(x) and x.is_cuda else torch.as_tensor(np.ascontiguousarray(x)).cuda(), lengths=lengths, owner={})
    B, L = sp.x.shape
    sp.ws.fill_(255)
    sp._call(3)
    sec = CleanStateCache._sections('siib', B, L, 0)
    if sec is None:
        _lib.check(-1, 'nele_metric_siib_clean_sections')
    rowstat, xdb, lst, info, _nprim, XL, lam = _section_rows(sp.ws, sec[3:10], B)      # sections 3 .. 9 (include/nele_hip.h)
    info = info.view(np.int32).copy()
    out = {'info': info, 'xdb': [], 'list': [], 'XL': [], 'rowstat': [], 'lam': []}
    for b in range(B):
        nt, na = int(info[b, 1]), int(info[b, 2])
        out['xdb'].append(xdb[b].view(np.float64)[:nt].copy())
        out['list'].append(lst[b].view(np.int32)[:na].copy())
        out['XL'].append(XL[b].view(np.float64).reshape(28, -1)[:, :na].copy())
        out['rowstat'].append(rowstat[b].view(np.float64).reshape(2, 28, 2)[0].copy())
        out['lam'].append(lam[b].view(np.float64).copy())
    return out


def siib_stages(x, y, lengths=None, phase2=True):
    """Diagnostic: nele_metric_siib_var in two calls (phase 1, then phase 2) on a workspace of its own (every byte 0xFF before the first call:
    what a kernel does not write reads as NaN / -1) -> dict of per-row numpy arrays, read through nele_metric_siib_sections.  Copied out
    after phase 1 (C is destroyed by the eigensolver and can only be read here), with na = info[b, 2] active frames, ncols = na - 14 stacked
    frames, signal 0 = clean x, 1 = degraded y, stacked row a = 28 k + j (k-th of 15 consecutive frames, band j):
      'info1' [B, 4] int = (M clamped to 40, frames of the tiled signal, na, status) as phase 1 leaves it.
      'rowstat'[b] [2, 28, 2] float64: per (signal, band) the minimum BEFORE masking and the mean AFTER masking.
      'XL'[b] [2, 28, na] float64: masked log band energies of the active frames of x then y (columns = the CLEAN signal's active list), row
          mean not yet removed: the consumers subtract rowstat[.., 1] on the fly, a_j[s] = XL[sig, j, s] - rowstat[sig, j, 1].
      'mu'[b] [2, 420] float64: window means mean_{t < ncols} a_j[t + k] of the stacked rows.
      'lagp'[b] [3, 4, 29, 28, 28] float64: [pair, frame segment, lag slot, j1, j2] partial sums over the segment's frames s of
          a_j1[s] b_j2[s + D] (all s with both indices in [0, na)); pair 0 = (x, x), 1 = (y, y), 2 = (x, y).  Slot D + 14 holds lag D; pairs 0
          and 1 fill slots 14 .. 28 only (slots 0 .. 13 stay 0xFF).  Segment seg covers frames [seg per, min(na, (seg + 1) per)) with
          per = ceil(ceil(na / 4) / g) g, g = 45 for pairs 0, 1 and 58 for pair 2; an empty segment holds zeros.  The lag product is
          (seg0 + seg1) + (seg2 + seg3).
      'C'[b] [420, 420] float64: Sxx / (ncols - 1), full, exactly symmetric.
      'S2'[b] [2, 420, 420] float64: Syy then (Sxy + Sxy^T) / 2, unscaled, UPPER triangle (row <= column) only: the strict lower triangle
          is never written (0xFF) and never read.
    Copied out after phase 2 on the same workspace:
      'lam'[b] [420] float64 ascending; 'U'[b] [420, 420] float64, ROW k = eigenvector k, and 'qpart'[b] [420, 14] float64 (7 column-tile
          partials of u_k^T Syy u_k, then 7 of u_k^T sym(Sxy) u_k) are meaningful for the KEPT components lam[k] > 1e-10 lam[419] only: in a
          64-row tile without a kept component U is zero and qpart stays 0xFF (NaN); the cut rows of a partly kept tile are unspecified.
      'raw' [B] float32 score, 'info' [B, 4] int as the call returns it.
    phase2=False stops after phase 1 (no eigensolver): the dict then holds the phase-1 buffers only."""
    sp = SiibSplit(x, y, lengths=lengths, owner={})
    B, L = sp.x.shape
    sp.ws.fill_(255)
    buf = (c_longlong * 30)()
    n = _lib.lib.nele_metric_siib_sections(B, L, buf, 10)
    if n != 10:
        _lib.check(n, 'nele_metric_siib_sections')
    sec = [(int(buf[3 * k]), int(buf[3 * k + 1]), int(buf[3 * k + 2])) for k in range(10)]
    sp.front()
    info1, rowstat, XL, mu, lagp, C, S2 = _section_rows(sp.ws, sec[:7], B)
    info1 = info1.view(np.int32).copy()
    out = {'info1': info1}
    out.update({k: [] for k in ('rowstat', 'XL', 'mu', 'lagp', 'C', 'S2')})
    if phase2:
        sp.back()
        lam, U, qpart = _section_rows(sp.ws, sec[7:], B)
        out.update({'info': sp.info.cpu().numpy(), 'raw': sp.raw.cpu().numpy(), 'lam': [], 'U': [], 'qpart': []})
    for b in range(B):
        na = max(int(info1[b, 2]), 0)
        out['rowstat'].append(rowstat[b].view(np.float64).reshape(2, 28, 2).copy())
        out['XL'].append(XL[b].view(np.float64).reshape(2, 28, -1)[:, :, :na].copy())
        out['mu'].append(mu[b].view(np.float64).reshape(2, 420).copy())
        out['lagp'].append(lagp[b].view(np.float64).reshape(3, 4, 29, 28, 28).copy())
        out['C'].append(C[b].view(np.float64).reshape(420, 420).copy())
        out['S2'].append(S2[b].view(np.float64).reshape(2, 420, 420).copy())
        if phase2:
            out['lam'].append(lam[b].view(np.float64).copy())
            out['U'].append(U[b].view(np.float64).reshape(420, 420).copy())
            out['qpart'].append(qpart[b].view(np.float64).reshape(420, 14).copy())
    return out


class _CleanSplit:
    """The clean-part protocol of SiibSplit, HaspiSplit and HasqiSplit.  A class names its CleanStateCache kind (its workspaces are
    KIND_split and, for a sub-batch, KIND_split_sub) and supplies, with whatever per-call arguments its clean_part() takes:
      _geom(*args)       the geometry key of the state phase 3 leaves, or None when this call's state must not be cached
      _phase3(*args)     the library call
      _sub(rows, *args)  -> (an object of the same class for batch rows ``rows`` on the sub-batch workspace, its own *args)"""

    KIND = None
    fs = 0                                      # what the section lists take as the sampling rate (SIIB: none)

    def _sub_kw(self, rows):
        return dict(lengths=None if self.lengths is None else self.lengths[rows], owner=self.owner, ws_kind=self.KIND + '_split_sub')

    def clean_part(self, cache=None, keys=None):
        """cache / keys: see _clean_part (the CleanStateCache kind is the class's KIND)."""
        return self._clean_part(cache, keys)

    def _clean_part(self, cache, keys, *args):
        """cache (CleanStateCache) + keys (one hashable per utterance, e.g. the file name): when every utterance's clean-signal state is
        cached it is copied into the workspace instead of being recomputed; when some are, phase 3 runs for the others only (a batch of
        their own on a second workspace) and everything is copied in; otherwise phase 3 runs for the batch and its utterances are stored.
        -> True when the state came from the cache."""
        geom = None if cache is None or keys is None else self._geom(*args)
        if geom is None:
            self._phase3(*args)
            return False
        kind, fs = self.KIND, self.fs
        B, L = self.x.shape
        full = list(keys)                       # a key stands for the clean waveform, its own length included
        slots = cache.lookup(kind, geom, full)
        if slots is not None:
            cache.restore(kind, geom, self.ws, B, L, fs, slots)
            return True
        rows = cache.missing(kind, geom, full)
        if rows is not None:
            # some utterances of the batch are known (a loop that re-draws its batches every epoch): phase 3 for the others only, as a batch
            # of their own on a second workspace, then everything comes from the cache (the kernels are batch-invariant: an utterance's state
            # does not depend on its row or on its batch-mates)
            sub, sub_args = self._sub(rows, *args)
            sub._phase3(*sub_args)
            if cache.store(kind, geom, sub.ws, len(rows), L, fs, [full[i] for i in rows]):
                slots = cache.lookup(kind, geom, full, count=False)
                if slots is not None:
                    cache.partial += 1
                    cache.restore(kind, geom, self.ws, B, L, fs, slots)
                    return True
        self._phase3(*args)
        cache.store(kind, geom, self.ws, B, L, fs, full)
        return False


class SiibSplit(_CleanSplit):
    """batch_siib in pieces.  front()/back(): wide kernels (VAD .. covariance) / latency-bound eigen-decomposition .. score, so
    that independent work can be enqueued in between on another stream.  clean_part()/degraded_part(y): split by data
    dependence - SIIB's Karhunen-Loeve basis comes from the clean signal alone, so VAD, the clean spectra, the covariance and its
    eigen-decomposition can run before the degraded signal exists."""

    KIND = 'siib'

    def __init__(self, x, y=None, lengths=None, owner=None, ws_kind='siib_split'):
        self.lengths = None
        self.owner = owner
        if y is None:
            self.x = x.contiguous().float()
            self.y = None
        else:
            self.x, self.y, _ = _pair(x, y)
        B, L = self.x.shape
        # own workspace: the clean-signal state must survive until degraded_part(), whatever else calls batch_siib() meanwhile
        # (``owner``: a dict held by the caller, e.g. one per trainer, that owns the workspace - released with the trainer)
        self.ws = _workspace(ws_kind, _lib.lib.nele_metric_siib_workspace_bytes(B, L), self.x.device, cache=owner)
        self.raw = torch.empty(B, device=self.x.device)
        self.mapped = torch.empty(B, device=self.x.device)
        self.info = torch.zeros((B, 4), dtype=torch.int32, device=self.x.device)
        self.lengths = _lens(lengths, self.x.device)

    def _call(self, phase):
        B, L = self.x.shape
        call('nele_metric_siib_var', ptr(self.x), ptr(self.y), ptr(self.lengths), B, L, ptr(self.ws), self.ws.numel(), ptr(self.raw),
             ptr(self.mapped), ptr(self.info), phase, stream())

    def front(self):
        self._call(1)

    def back(self):
        self._call(2)
        return self.raw, self.mapped

    def _geom(self):
        return ('L', self.x.shape[1])

    def _phase3(self):
        self._call(3)

    def _sub(self, rows):
        return SiibSplit(self.x[rows], **self._sub_kw(rows)), ()

    def degraded_part(self, y):
        assert y.shape == self.x.shape
        self.y = y.contiguous().float()
        self._call(4)
        return self.raw, self.mapped


def batch_siib(x, y, return_info=False, lengths=None):
    """clean x [B,L], degraded y [B,L] (16 kHz) -> (raw [B] bits/s, mapped [B]); the replication rule of
    intel.py:93-97 is applied per utterance on the device.  info [B,4] = (M, tiled frames, active frames, status)."""
    sp = SiibSplit(x, y, lengths=lengths, ws_kind='siib')
    sp._call(0)
    if return_info:
        return sp.raw, sp.mapped, sp.info
    return sp.raw, sp.mapped


def _siib_checked(x, y):
    raw, mapped, info = batch_siib(x, y, return_info=True)
    st = int(info[0, 3])
    if st & 8:
        raise ValueError("SIIB: not enough active speech frames")       # pysiib / reference raise here
    if st & 1:
        raise ValueError("SIIB: replication factor above the supported maximum")
    return raw, mapped


def SIIB_Wrapper_raw_harvard(x, y, fs):
    assert fs == 16000
    return float(_siib_checked(x, y)[0][0])


def SIIB_Wrapper_harvard(x, y, fs):
    assert fs == 16000
    return float(_siib_checked(x, y)[1][0])


def _hl6(HL):
    """Audiogram argument of the reference's pyHASPI functions (HL = np.zeros(6) by default) -> ctypes double[6] or None (normal hearing)."""
    if HL is None:
        return None
    v = [float(t) for t in np.asarray(HL, dtype=np.float64).reshape(-1)]
    if len(v) != 6:
        raise ValueError('HL must hold the six audiogram values at 250, 500, 1000, 2000, 4000, 6000 Hz (pyhaspi2.py:780)')
    if not any(v):
        return None
    return (ctypes.c_double * 6)(*v)


def batch_haspi(x, y, fs=16000, dither=None, seed=None, return_info=False, lengths=None, HL=None):
    """clean x [B,L], degraded y [B,L] -> (raw HASPI v2 [B], mapped [B]).
    HL: audiogram of the listener (six values in dB HL, pyhaspi2.py:76, 779-807); None / zeros = normal hearing (what the loop uses).
    dither: None -> no IHC firing jitter (deterministic score); True -> standard normals drawn on the device
    (torch generator, optional ``seed``) as the reference does with np.random.randn (pyhaspi2.py:362-365); or a
    float64 tensor [B,2,nsub,32] whose row k perturbs the k-th active frame (used by the parity tests)."""
    x, y, _ = _pair(x, y)
    B, L = x.shape
    nsub = _lib.lib.nele_metric_haspi_nsub(L, fs)
    if dither is True:
        g = None
        if seed is not None:
            g = torch.Generator(device=x.device)
            g.manual_seed(int(seed))
        dither = torch.randn((B, 2, nsub, 32), dtype=torch.float64, device=x.device, generator=g)
    if dither is not None:
        if tuple(dither.shape) != (B, 2, nsub, 32) or dither.dtype != torch.float64:
            raise ValueError("batch_haspi: dither must be float64 [B, 2, %d, 32]" % nsub)
        dither = dither.to(x.device).contiguous()
    nb = _lib.lib.nele_metric_haspi_workspace_bytes(B, L, fs)
    ws = _workspace('haspi', nb, x.device)
    raw = torch.empty(B, device=x.device)
    mapped = torch.empty(B, device=x.device)
    info = torch.zeros((B, 2), dtype=torch.int32, device=x.device)
    if lengths is not None:
        lengths = torch.as_tensor(lengths).to(device=x.device, dtype=torch.int32).contiguous()
    hl = _hl6(HL)
    if hl is None:
        call('nele_metric_haspi_var', ptr(x), ptr(y), ptr(lengths), B, L, int(fs), ptr(dither), ptr(ws), ws.numel(), ptr(raw), ptr(mapped), ptr(info), 0,
             stream())
    else:
        call('nele_metric_haspi_var_hl', ptr(x), ptr(y), ptr(lengths), B, L, int(fs), ptr(dither), hl, 0, ptr(ws), ws.numel(), ptr(raw), ptr(mapped),
             ptr(info), 0, stream())
    if return_info:
        return raw, mapped, info
    return raw, mapped


def haspi_stages(x, y, fs, lengths=None, dither=None, HL=None):
    """Diagnostic: batch_haspi on a workspace of its own (every byte 0xFF before the call: what a kernel does not write reads as NaN / -1),
    ONE nele_metric_haspi_var_hl call at phase 0 -> (raw float32 numpy [B], info int32 numpy [B, 2] = (n_active, status), stages): the
    workspace read through nele_metric_haspi_sections.  stages[name][b] is row b's array, cut to the row's own sizes (n24 samples at
    24 kHz, nsub = ceil(n24 / 9) frames, na = n_active frames above the silence gate):
      'r24' [2, n24] float32: x then y at 24 kHz WITH the RMS-restore gain (float32(gain * stored), the product the middle-ear kernel forms);
      'rinfo' [2, 4] float32; 'mid' [2, n24]; 'ctl' [2, n24, 32] float32 control |u|^2 without the filter gain; 'bw' [2, 32]; 'shift' [32];
      'env' [2, n24, 32] float32 dB SL before IHC adaptation; 'lp' [2, nsub, 32] in FRAME order (the group-space rows of the workspace are
      un-shuffled here: frame i of channel c = row i - di(c), rows below 0 are zero); 'index' [na] the active frames, from 'act' [nsub];
      'cep' [2, 6, na] MEAN-REMOVED (the kernel stores the sequences mean-removed with cmean = 0; stored - cmean is returned, which is the
      mean-removed sequence whichever of the two holds the mean); 'cmean' [2, 6] as stored; 'xf' [na, 50]; 'cm' [5, 10] (bases 1..5);
      'loss' [2, 5, 32] (shared by the rows)."""
    x, y, _ = _pair(x, y)
    B, L = x.shape
    fs = int(fs)
    nsub = _lib.lib.nele_metric_haspi_nsub(L, fs)
    if dither is not None:
        dither = torch.as_tensor(dither)
        if tuple(dither.shape) != (B, 2, nsub, 32) or dither.dtype != torch.float64:
            raise ValueError("haspi_stages: dither must be float64 [B, 2, %d, 32]" % nsub)
        dither = dither.to(x.device).contiguous()
    ws = torch.full((int(_lib.lib.nele_metric_haspi_workspace_bytes(B, L, fs)),), 255, dtype=torch.uint8, device=x.device)
    raw = torch.empty(B, device=x.device)
    info = torch.full((B, 2), -1, dtype=torch.int32, device=x.device)
    lens = _lens(lengths, x.device)
    call('nele_metric_haspi_var_hl', ptr(x), ptr(y), ptr(lens), B, L, fs, ptr(dither), _hl6(HL), 0, ptr(ws), ws.numel(), ptr(raw), None, ptr(info), 0,
         stream())
    buf = (c_longlong * 45)()
    n = _lib.lib.nele_metric_haspi_sections(B, L, fs, buf, 15)
    if n != 15:
        _lib.check(n, 'nele_metric_haspi_sections')
    sec = [(int(buf[3 * k]), int(buf[3 * k + 1]), int(buf[3 * k + 2])) for k in range(15)]
    r24, mid, bw, shift, rinfo, env, ctl, lp, act, winfo, cep, cmean, xf, cm = _section_rows(ws, sec[:14], B)
    loss = ws[sec[14][0]:sec[14][0] + sec[14][2]].cpu().numpy().view(np.float64).reshape(2, 5, 32).copy()
    info = info.cpu().numpy()
    lens = np.full(B, L) if lengths is None else np.minimum(np.asarray(torch.as_tensor(lengths).cpu()), L)
    names = ('r24', 'rinfo', 'mid', 'ctl', 'bw', 'shift', 'env', 'lp', 'index', 'cep', 'cmean', 'xf', 'cm', 'act', 'info')
    out = {k: [] for k in names}
    out['loss'] = loss
    for b in range(B):
        n24 = int(lens[b]) if fs == 24000 else int(np.ceil(float(int(lens[b])) * (24000.0 / fs)))
        ns = -(-n24 // 9)
        ri = rinfo[b].view(np.float32).reshape(2, 4).copy()
        sh = shift[b].view(np.int32).copy()
        a = act[b].view(np.int32)[:ns].copy()
        wi = winfo[b].view(np.int32).copy()
        na = max(int(wi[0]), 0)
        out['rinfo'].append(ri)
        out['r24'].append(ri[:, 2:3] * r24[b].view(np.float32).reshape(2, -1)[:, :n24])        # float32 product, as haspi_midear_par_kernel forms it
        out['mid'].append(mid[b].view(np.float64).reshape(2, -1)[:, :n24].copy())
        out['ctl'].append(ctl[b].view(np.float32).reshape(2, -1, 32)[:, :n24].copy())
        out['env'].append(env[b].view(np.float32).reshape(2, -1, 32)[:, :n24].copy())
        out['bw'].append(bw[b].view(np.float64).reshape(2, 32).copy())
        out['shift'].append(sh)
        # group-space rows -> frame order (hp_lp_di / hp_lp_at of csrc/haspi.hip)
        di = (((26 - sh) % 9 + 9) % 9 + sh - 26) // 9
        graw = lp[b].view(np.float64).reshape(2, nsub + 4, 32)
        g = np.arange(ns)[:, None] - di[None, :]                                                # [ns, 32]
        fr = graw[:, np.clip(g, 0, nsub + 3), np.arange(32)[None, :]]
        out['lp'].append(np.where((g >= 0)[None], fr, 0.0))
        out['act'].append(a)
        order = np.argsort(a, kind='stable')
        out['index'].append(order[a[order] >= 0])                                               # frame of the k-th active position
        out['info'].append(wi)
        cm_ = cmean[b].view(np.float64).reshape(2, 6).copy()
        out['cmean'].append(cm_)
        out['cep'].append(cep[b].view(np.float64).reshape(2, 6, nsub)[:, :, :na] - cm_[:, :, None])
        out['xf'].append(xf[b].view(np.float64).reshape(nsub, 64)[:na, :50].copy())
        out['cm'].append(cm[b].view(np.float64).reshape(6, 10)[1:].copy())
    return raw.cpu().numpy(), info, out


def haspi_dither_rows(utt_ids, seed, L, fs=16000, device=None):
    """Dither rows [B, 2, nsub, 32] float64 for batch_haspi / HaspiSplit, drawn per UTTERANCE ID (pyhaspi2.py:362-365 draws
    np.random.randn rows on every call; here a row is a pure function of (seed, id, signal, frame, channel), so an utterance is
    scored alike on any rank and in any batch - SURVEY 8e).  utt_ids: [B] integers."""
    ids = torch.as_tensor(utt_ids)
    device = device or (ids.device if ids.is_cuda else 'cuda')
    ids = ids.to(device=device, dtype=torch.int64).contiguous()
    B = ids.shape[0]
    nsub = _lib.lib.nele_metric_haspi_nsub(int(L), int(fs))
    out = torch.empty((B, 2, nsub, 32), dtype=torch.float64, device=ids.device)
    call('nele_haspi_dither_rows', ptr(ids), int(seed) & 0xFFFFFFFFFFFFFFFF, B, nsub, ptr(out), stream())
    return out


class HaspiSplit(_CleanSplit):
    """batch_haspi split by data dependence: clean_part() runs the whole reference-signal chain (ear model, envelope filter,
    silence gate, group-delay shifts, cepstra, modulation filters) before the degraded signal exists; degraded_part(y) does the same
    for y and correlates.  Own workspace: the clean-signal state must survive until degraded_part()."""

    KIND = 'haspi'

    def __init__(self, x, fs=16000, lengths=None, owner=None, ws_kind='haspi_split'):
        self.x = x.contiguous().float()
        self.fs = int(fs)
        self.owner = owner
        B, L = self.x.shape
        self.lengths = None if lengths is None else lengths.to(device=self.x.device, dtype=torch.int32).contiguous()
        self.ws = _workspace(ws_kind, _lib.lib.nele_metric_haspi_workspace_bytes(B, L, self.fs), self.x.device, cache=owner)
        self.raw = torch.empty(B, device=self.x.device)
        self.mapped = torch.empty(B, device=self.x.device)
        self.info = torch.zeros((B, 2), dtype=torch.int32, device=self.x.device)

    def _call(self, y, dither, phase):
        B, L = self.x.shape
        call('nele_metric_haspi_var', ptr(self.x), ptr(y), ptr(self.lengths), B, L, self.fs, ptr(dither), ptr(self.ws), self.ws.numel(),
             ptr(self.raw), ptr(self.mapped), ptr(self.info), phase, stream())

    def _geom(self, dither, dither_tag):
        if dither is not None and dither_tag is None:
            return None
        return ('L', self.x.shape[1], 'fs', self.fs, 'dither', dither_tag)

    def _phase3(self, dither, dither_tag):
        self._call(None, dither, 3)

    def _sub(self, rows, dither, dither_tag):
        return (HaspiSplit(self.x[rows], fs=self.fs, **self._sub_kw(rows)), (None if dither is None else dither[rows].contiguous(), dither_tag))

    def clean_part(self, dither=None, cache=None, keys=None, dither_tag=None):
        """cache / keys: see _CleanSplit._clean_part (CleanStateCache kind 'haspi').  ``dither_tag``: hashable that identifies the reference's
        dither rows (None = no dither; e.g. ('utterance', seed) for rows drawn per utterance id) - a cached state is only valid for the
        dither it was computed with; a dither with no tag is never cached."""
        return self._clean_part(cache, keys, dither, dither_tag)

    def degraded_part(self, y, dither=None):
        assert y.shape == self.x.shape
        self.y = y.contiguous().float()
        self._call(self.y, dither, 4)
        return self.raw, self.mapped


QUALITY_FIELDS = ('haspi', 'CepCorr', 'cov3_low', 'cov3_mid', 'cov3_high', 'hasqi', 'Nonlin', 'Linear', 'BMsync5', 'Dloud', 'Dslope', 'avecov')


def batch_haspi_quality(x, y, fs=16000, lengths=None, noise=True, seed=None, alpha=-1.0, return_info=False, HL=None, itype=0):
    """reference x [B,L], processed y [B,L] -> float64 [B, 12] (columns QUALITY_FIELDS): HASPI version 1 (pyhaspi2.py:109-157) and
    HASQI v2 (pyhaspi2.py:32-74) from one launch chain.  noise: the reference's eb_BMaddnoise (device generator, ``seed`` or a fresh
    one per call); False = none (deterministic, the parity tests).  HL: audiogram (six values in dB HL); with a loss the two models
    differ in how the reference signal is heard (pyhaspi2.py:1162-1166): itype 0 -> the `haspi` columns are valid, itype 2 -> the
    `hasqi_v2` columns."""
    x, y, _ = _pair(x, y)
    B, L = x.shape
    ws = _workspace('haspi_quality', _lib.lib.nele_metric_haspi_quality_workspace_bytes(B, L, int(fs)), x.device)
    out = torch.empty((B, len(QUALITY_FIELDS)), dtype=torch.float64, device=x.device)
    info = torch.zeros((B, 4), dtype=torch.int32, device=x.device)
    if lengths is not None:
        lengths = torch.as_tensor(lengths).to(device=x.device, dtype=torch.int32).contiguous()
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if noise else 0
    hl = _hl6(HL)
    if hl is None:
        call('nele_metric_haspi_quality', ptr(x), ptr(y), ptr(lengths), B, L, int(fs), int(bool(noise)), int(seed), float(alpha), ptr(ws), ws.numel(),
             ptr(out), ptr(info), stream())
    else:
        call('nele_metric_haspi_quality_hl', ptr(x), ptr(y), ptr(lengths), B, L, int(fs), int(bool(noise)), int(seed), float(alpha), hl, int(itype),
             ptr(ws), ws.numel(), ptr(out), ptr(info), stream())
    return (out, info) if return_info else out


HASQI_FIELDS = ('Combined', 'Nonlin', 'Linear', 'CepCorr', 'BMsync5', 'Dloud', 'Dslope')
QUALITY_TARGET_FIELDS = ('Nonlin', 'Linear')          # D_Qua's two targets when it is trained on HASQI (quality.HasqiScorer)
_HASQI_NOISE = {False: 0, None: 0, 0: 0, True: 1, 1: 1, 'row': 1, 'utterance': 2, 2: 2}


class HasqiSplit(_CleanSplit):
    """HASQI v2 (pyhaspi2.py:32-74) of a batch, split by data dependence like HaspiSplit: clean_part() runs everything that needs the
    reference x alone (its ear model with the basilar-membrane motion, group-delay shifts, smoothed envelope, mean squares, segment
    loudness) and degraded_part(y) - any number of times - the chain of y, the cross-covariance and the scores: float64 [B, 7]
    (HASQI_FIELDS; a new tensor per call), status in ``info`` [B, 4].
    noise: False | True (eb_BMaddnoise keyed by (seed, row of the batch)) | 'utterance' (keyed by (seed, utt_ids[b]): an utterance is
    scored alike at any row of any batch on any rank).  The noise of x is part of what clean_part() leaves.  HL: audiogram heard by both
    signals.  Own workspace: the clean-signal state must survive until degraded_part()."""

    KIND = 'hasqi'

    def __init__(self, x, fs=16000, lengths=None, noise=False, seed=0, utt_ids=None, HL=None, owner=None, ws_kind='hasqi_split'):
        self.x = x.contiguous().float()
        self.fs = int(fs)
        self.owner = owner
        if noise not in _HASQI_NOISE:
            raise ValueError("HASQI: noise must be False, True or 'utterance'")
        self.noise, self.seed, self.HL = _HASQI_NOISE[noise], int(seed) & 0xFFFFFFFFFFFFFFFF, HL
        self.hl = _hl6(HL)
        B, L = self.x.shape
        self.utt_ids = None
        if self.noise == 2:
            if utt_ids is None:
                raise ValueError("HASQI: noise='utterance' needs utt_ids")
            self.utt_ids = torch.as_tensor(utt_ids).to(device=self.x.device, dtype=torch.int64).contiguous()
            if tuple(self.utt_ids.shape) != (B,):
                raise ValueError('HASQI: utt_ids must hold one id per row')
        self.lengths = _lens(lengths, self.x.device)
        self.ws = _workspace(ws_kind, _lib.lib.nele_metric_hasqi_workspace_bytes(B, L, self.fs), self.x.device, cache=owner)
        self.info = torch.zeros((B, 4), dtype=torch.int32, device=self.x.device)

    def _call(self, y, phase, out=None):
        B, L = self.x.shape
        call('nele_metric_hasqi_var', ptr(self.x), ptr(y), ptr(self.lengths), B, L, self.fs, self.hl, self.noise, self.seed, ptr(self.utt_ids),
             ptr(self.ws), self.ws.numel(), ptr(out), ptr(self.info), phase, stream())

    def _geom(self):
        # a cached state is valid for the noise it holds: none, or the per-utterance one of this seed; row-keyed noise is never cached
        if self.noise == 1:
            return None
        return ('L', self.x.shape[1], 'fs', self.fs, 'noise', (self.noise, self.seed) if self.noise else 0, 'HL', None if self.hl is None else tuple(self.hl))

    def _phase3(self):
        self._call(None, 3)

    def _sub(self, rows):
        return HasqiSplit(self.x[rows], fs=self.fs, noise=self.noise, seed=self.seed, utt_ids=None if self.utt_ids is None else self.utt_ids[rows],
                          HL=self.HL, **self._sub_kw(rows)), ()

    def degraded_part(self, y):
        assert y.shape == self.x.shape
        self.y = y.contiguous().float()
        out = torch.empty((self.x.shape[0], len(HASQI_FIELDS)), dtype=torch.float64, device=self.x.device)
        self._call(self.y, 4, out)
        return out


def batch_hasqi(x, y, fs=16000, lengths=None, noise=False, seed=0, utt_ids=None, HL=None, return_info=False):
    """reference x [B,L], processed y [B,L] -> float64 [B, 7] (HASQI_FIELDS): hasqi_v2 (pyhaspi2.py:32-74) alone, one launch chain
    (phase 0 of nele_metric_hasqi_var).  noise / seed / utt_ids / HL: see HasqiSplit.  info [B,4] = (segments above threshold of
    eb_melcor, status, of the covariance, loudness bins); status bits 1 / 2 (signal below threshold) make a row NaN."""
    x, y, _ = _pair(x, y)
    sp = HasqiSplit(x, fs=fs, lengths=lengths, noise=noise, seed=seed, utt_ids=utt_ids, HL=HL, ws_kind='hasqi')
    out = torch.empty((x.shape[0], len(HASQI_FIELDS)), dtype=torch.float64, device=x.device)
    sp._call(y, 0, out)
    return (out, sp.info) if return_info else out


def haspi_quality_stages(x, y, fs, lengths=None, HL=None, itype=0, noise=False, seed=0, split=None, utt_ids=None):
    """Diagnostic (tests only; nothing in training calls it): HASPI v1 / HASQI v2 on a workspace of its own (every byte 0xFF before the
    call: what a kernel does not write reads as NaN / -1) -> (out float64 numpy, info int32 numpy [B, 4], stages): the workspace read
    through nele_metric_haspi_quality_sections.  split=None: one nele_metric_haspi_quality[_hl] call, out [B, 12] (QUALITY_FIELDS);
    split='phase0': one nele_metric_hasqi_var call at phase 0, split='3+4': its phase 3 then its phase 4 on the same workspace, out [B, 7]
    (HASQI_FIELDS; both hear HL with itype 2).  noise: False | True | 'utterance' (the split forms, with utt_ids).
    stages[name][b] is row b's array, cut to the row's own n24 samples at 24 kHz and nseg = 1 + n24 // 384 + (n24 - 192) // 384 segments:
      'r24' [2, n24] float32 WITH the RMS-restore gain (as haspi_stages); 'rinfo' [2, 4] float32; 'bw' [2, 32]; 'shift' [32] int32;
      'env' [2, n24, 32] float32 the ADAPTED envelope in dB SL and 'bm' [2, n24, 32] float32 the basilar-membrane motion, both BEFORE the
      group-delay shift; 'sse' / 'ssp' [2, chunks of the row, 32] sums of |u|^2 of the signal / control bank without the filter gain;
      'sm' [2, nseg, 32]; 'cov', 'msx', 'msy' [nseg, 32]; 'segl' [2, nseg]; 'qinfo' [4] int32; 'sl' [2, 32];
    and, shared by the rows, 'corr' [2, 49] and 'loss' [2, 5, 32]."""
    x, y, _ = _pair(x, y)
    B, L = x.shape
    fs = int(fs)
    if split not in (None, 'phase0', '3+4'):
        raise ValueError("haspi_quality_stages: split must be None, 'phase0' or '3+4'")
    if noise not in _HASQI_NOISE:
        raise ValueError("haspi_quality_stages: noise must be False, True or 'utterance'")
    nz = _HASQI_NOISE[noise]
    hl = _hl6(HL)
    if split is None and nz == 2:
        raise ValueError('haspi_quality_stages: per-utterance noise exists in the split entry point only')
    if split is not None and hl is not None and itype != 2:
        raise ValueError('haspi_quality_stages: nele_metric_hasqi_var hears the loss with itype 2 only')
    ids = None
    if nz == 2:
        ids = torch.as_tensor(utt_ids).to(device=x.device, dtype=torch.int64).contiguous()
    ws = torch.full((int(_lib.lib.nele_metric_haspi_quality_workspace_bytes(B, L, fs)),), 255, dtype=torch.uint8, device=x.device)
    out = torch.full((B, len(QUALITY_FIELDS) if split is None else len(HASQI_FIELDS)), -1.0, dtype=torch.float64, device=x.device)
    info = torch.full((B, 4), -1, dtype=torch.int32, device=x.device)
    lens = _lens(lengths, x.device)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    if split is None:
        if hl is None:
            call('nele_metric_haspi_quality', ptr(x), ptr(y), ptr(lens), B, L, fs, nz, seed, -1.0, ptr(ws), ws.numel(), ptr(out), ptr(info), stream())
        else:
            call('nele_metric_haspi_quality_hl', ptr(x), ptr(y), ptr(lens), B, L, fs, nz, seed, -1.0, hl, int(itype), ptr(ws), ws.numel(), ptr(out),
                 ptr(info), stream())
    else:
        for phase in ((0,) if split == 'phase0' else (3, 4)):
            call('nele_metric_hasqi_var', ptr(x) if phase != 4 else None, ptr(y) if phase != 3 else None, ptr(lens), B, L, fs, hl, nz, seed, ptr(ids),
                 ptr(ws), ws.numel(), ptr(out), ptr(info), phase, stream())
    buf = (c_longlong * 51)()
    n = _lib.lib.nele_metric_haspi_quality_sections(B, L, fs, buf, 17)
    if n != 17:
        _lib.check(n, 'nele_metric_haspi_quality_sections')
    sec = [(int(buf[3 * k]), int(buf[3 * k + 1]), int(buf[3 * k + 2])) for k in range(17)]
    r24, rinfo, bw, shift, env, bm, sse, ssp, sm, cov, msx, msy, segl, qinfo, sl = _section_rows(ws, sec[:15], B)
    corr, loss = (ws[o:o + nb].cpu().numpy().view(np.float64).copy() for (o, _st, nb) in sec[15:])
    lens = np.full(B, L) if lengths is None else np.minimum(np.asarray(torch.as_tensor(lengths).cpu()), L)
    n24p = sec[0][2] // 8
    lc = 1536                                            # GS_LC of csrc/haspi.hip; longer chunks beyond GS_MAXC = 160 of them
    while -(-n24p // lc) > 160:
        lc += 1536
    st = {k: [] for k in ('r24', 'rinfo', 'bw', 'shift', 'env', 'bm', 'sse', 'ssp', 'sm', 'cov', 'msx', 'msy', 'segl', 'qinfo', 'sl')}
    st['corr'] = corr.reshape(2, 64)[:, :49].copy()
    st['loss'] = loss.reshape(2, 5, 32)
    for b in range(B):
        n24 = int(lens[b]) if fs == 24000 else int(np.ceil(float(int(lens[b])) * (24000.0 / fs)))
        nseg, nchk = 1 + n24 // 384 + (n24 - 192) // 384, -(-n24 // lc)
        ri = rinfo[b].view(np.float32).reshape(2, 4).copy()
        st['rinfo'].append(ri)
        st['r24'].append(ri[:, 2:3] * r24[b].view(np.float32).reshape(2, -1)[:, :n24])
        st['bw'].append(bw[b].view(np.float64).reshape(2, 32).copy())
        st['shift'].append(shift[b].view(np.int32).copy())
        st['env'].append(env[b].view(np.float32).reshape(2, -1, 32)[:, :n24].copy())
        st['bm'].append(bm[b].view(np.float32).reshape(2, -1, 32)[:, :n24].copy())
        st['sse'].append(sse[b].view(np.float64).reshape(2, -1, 32)[:, :nchk].copy())
        st['ssp'].append(ssp[b].view(np.float64).reshape(2, -1, 32)[:, :nchk].copy())
        st['sm'].append(sm[b].view(np.float64).reshape(2, -1, 32)[:, :nseg].copy())
        for k, a in (('cov', cov), ('msx', msx), ('msy', msy)):
            st[k].append(a[b].view(np.float64).reshape(-1, 32)[:nseg].copy())
        st['segl'].append(segl[b].view(np.float64).reshape(2, -1)[:, :nseg].copy())
        st['qinfo'].append(qinfo[b].view(np.int32).copy())
        st['sl'].append(sl[b].view(np.float64).reshape(2, 32).copy())
    return out.cpu().numpy(), info.cpu().numpy(), st


def _quality_checked(x, fx, y, fy, alpha=-1.0, HL=None, itype=0):
    if fx != fy:
        raise ValueError('haspi / hasqi_v2: both signals must have the same sampling rate here (the reference resamples each to 24 kHz)')
    L = min(len(x), len(y))
    out, info = batch_haspi_quality(x[:L], y[:L], fx, alpha=alpha, return_info=True, HL=HL, itype=itype)
    st = int(info[0, 1])
    if st & 1:
        raise Exception('Function eb_melcor: Signal below threshold, outputs set to 0.')        # pyhaspi2.py:723-724
    return out[0].cpu().numpy(), st


def haspi(x, fx, y, fy, HL=None, alpha=-1.0):
    """pyhaspi2.py:109-157 (HASPI version 1): -> (Intel, raw = [CepCorr, cov3 low, mid, high]).  HL: audiogram of the listener."""
    o, st = _quality_checked(x, fx, y, fy, alpha, HL=HL, itype=0)
    if st & 2:
        raise Exception('Function eb_3LevelCovary: Signal below threshold, outputs set to 0.')    # pyhaspi2.py:427-428
    return float(o[0]), o[1:5].copy()


def hasqi_v2(x, fx, y, fy, HL=None):
    """pyhaspi2.py:32-74: -> (Combined, Nonlin, Linear, raw = [CepCorr, BMsync5, Dloud, Dslope]).  HL: audiogram (both signals are heard
    with it: eq = 2, pyhaspi2.py:41-43)."""
    o, st = _quality_checked(x, fx, y, fy, HL=HL, itype=2)
    if st & 2:
        raise TypeError("'int' object is not subscriptable")                                       # eb_AveCovary2's (0, 0) return at pyhaspi2.py:54
    return float(o[5]), float(o[6]), float(o[7]), [float(o[1]), float(o[8]), float(o[9]), float(o[10])]


def haspi_v2(x, fx, y, fy, HL=None):
    """pyhaspi2.py:76-107: -> Intel (the modulation-band correlations `raw` stay on the device).  The reference dithers every call
    (pyhaspi2.py:362-365): so does this wrapper; batch_haspi(dither=None) is the deterministic form."""
    if fx != fy:
        raise ValueError('haspi_v2: both signals must have the same sampling rate here (the reference resamples each to 24 kHz)')
    L = min(len(x), len(y))
    raw, mapped, info = batch_haspi(x[:L], y[:L], fx, dither=True, return_info=True, HL=HL)
    if int(info[0, 1]):
        raise Exception('Function ebm_CepCoef: Signal below threshold')     # pyhaspi2.py:357-358
    return float(raw[0])


def _haspi_checked(x, y, fs):
    raw, mapped, info = batch_haspi(x, y, fs, dither=True, return_info=True)
    if int(info[0, 1]):
        raise Exception('Function ebm_CepCoef: Signal below threshold')     # pyhaspi2.py:357-358
    return raw, mapped


def HASPI_Wrapper_raw_harvard(x, y, fs):
    return float(_haspi_checked(x, y, fs)[0][0])


def HASPI_Wrapper_harvard(x, y, fs):
    return float(_haspi_checked(x, y, fs)[1][0])


def ESTOI_Wrapper_raw_harvard(x, y, fs):
    assert fs == 16000
    return float(batch_estoi(x, y)[0][0])


def ESTOI_Wrapper_harvard(x, y, fs):
    assert fs == 16000
    return float(batch_estoi(x, y)[1][0])


def mapping_ESTOI_harvard(x):
    return 1 / (1 + np.exp(-8.0 * (x - 0.25)))


def mapping_SIIB_harvard(x):
    return 1 / (1 + np.exp(-0.06 * (x - 32)))


def mapping_HASPI_harvard(x):
    return 1 / (1 + np.exp(-0.95 * (x - 2.8)))
