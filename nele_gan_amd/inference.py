"""Enhancement path of the reference ``inference.py`` (inference.py:79-117), batched on the GPU:
features -> G (eval) -> mask * beta2 -> resynthesis -> enh / rms(enh) * 0.03 -> PCM_16.

``Enhancer.enhance``         one padded batch resident in HBM (optional per-utterance lengths), on the current stream
``Enhancer.enhance_stream``  a sequence of batches with several of them in flight on their own streams: the noise branch of a batch
                             (STFT -> IMCRA, a scan that is serial over frames and fills a fraction of the chip) runs under the
                             generator of the batch before it; results come out in order, bit-identical to ``enhance``
``enhance_files``            the reference's loop over a file list (inference.py:79-117): files of any lengths are decoded on a
                             small thread pool, padded side by side in batches, staged through pinned host buffers, enhanced with
                             ``enhance_stream`` and written as '<name>@1.wav' PCM_16; with torch.distributed initialised every
                             rank takes a contiguous shard of the list (BASELINE configs[4]: data-parallel enhancement, pure
                             replicas, no collective).
"""
import collections
import os

import torch

from . import audio_util as au
from . import dist as ndist
from . import model as M
from . import ops
from . import _lib

p_power = (1 / 6)
inv_p = 6
fs = 16000


class Enhancer:
    def __init__(self, chkpt_path=None, device='cuda', G=None, norm=None):
        """norm: the energy normalisation of mask -> alpha^2 - 'utterance' (inference.py:99-104: sums over the whole utterance) or
        'prefix' (sums over the frames up to each frame: what realtime.RealtimeEnhancer emits; train with
        GanTrainer(norm='prefix')).  None: what the checkpoint records ('enhance-norm'), else 'utterance'.  The final
        enh / rms(enh) * 0.03 and PCM_16 are the same in both modes."""
        if norm is not None:
            M.check_norm(norm, 'Enhancer')
        self.device = _lib.norm_dev(device)
        self.G = G if G is not None else M.Generator_Conv1D_cLN()
        recorded = 'utterance'
        if chkpt_path is not None:
            ck = torch.load(chkpt_path, map_location='cpu')
            self.G.load_state_dict(ck['enhance-model'])                                           # inference.py:71-72
            recorded = M.check_norm(ck.get('enhance-norm', 'utterance'), 'Enhancer (checkpoint)')
        self.norm = recorded if norm is None else norm
        self.G = self.G.to(self.device)
        self.G.eval()
        # An Enhancer that owns its generator (loaded from a checkpoint, never trained through this object) writes the weight layouts once and
        # keeps them: plain enhance() then skips the three weight-layout launches per batch as enhance_stream always did (0.06 of 1.9 ms and
        # 187 MB of traffic per 128 x 8 s batch).  A generator handed in (G=trainer.G) may be stepped between calls: its layouts are redone.
        self._own_G = G is None
        self._frozen_precision = None
        self._slots = []                # streams of enhance_stream, created on first use and kept (the runtime maps streams to hardware queues once)

    def _enhance_impl(self, clean_wav, noise_wav, pcm16, lengths, rms_target=0.030):
        if self._own_G and not torch.cuda.is_current_stream_capturing() and (not self.G._weights_frozen or self._frozen_precision != self.G.precision):
            torch.cuda.current_stream(self.device).wait_event(self.G.freeze_weights(self.device))
            self._frozen_precision = self.G.precision
        lengths = au._i32(lengths, self.device)
        frames = au.frames_of(lengths)
        clean_spec, clean_band = au.stft_band(clean_wav, p_power, lengths=lengths)
        noise_band = au.noise_band(noise_wav, p_power, lengths=lengths, frames=frames)
        mask = self.G(clean_band, noise_band)
        alpha2 = M.normed_alpha2(mask, clean_band, inv_p, frames=frames, norm=self.norm)
        return au.gain_istft(alpha2, clean_spec, rms_target=rms_target, pcm16=pcm16, frames=frames)

    @torch.no_grad()
    def enhance(self, clean_wav, noise_wav, pcm16=True, lengths=None, rms_target=0.030):
        """clean_wav, noise_wav [B,L] -> enhanced wav [B, 256*(T-1)] at RMS 0.03 (inference.py:99-115).
        lengths [B] (optional): samples of each utterance inside the padded batch; row b of the result then holds
        256 * (lengths[b] // 256) samples followed by zeros, and its RMS is taken over those samples.
        rms_target = 0: no final gain (with norm='prefix' and pcm16=False: the signal the real-time path emits)."""
        return self._enhance_impl(clean_wav, noise_wav, pcm16, lengths, rms_target)

    @torch.no_grad()
    def enhance_stream(self, batches, inflight=4, pcm16=True):
        """batches: iterable of (clean_wav [B,L], noise_wav [B,L]) or (clean_wav, noise_wav, lengths) device tensors (shapes may differ
        from batch to batch).  Generator of the enhanced batches, in order; each equals ``enhance`` of the same batch bit for bit.

        Up to ``inflight`` batches are enqueued before the oldest result is handed out, each on a stream of its own with its own set
        of generator activation buffers (``Generator_Conv1D_cLN.buffer_slot``); the generator's weight layouts are written once
        (``freeze_weights``) and only read afterwards.  One batch by itself is a chain of kernels of which the IMCRA scan (serial over
        the frames, 1 / 8 .. 1 / 4 of the chip) and the per-utterance tails leave most of the GPU idle: with several batches in flight those
        phases run under another batch's generator (inference.py:79-117 is a loop over independent files).  Throughput = batches in
        flight / a batch's latency as long as every batch sits on a hardware queue of its own; the runtime has four, so the default is
        four batches - three side streams and the caller's own stream (round 6: 102 k -> 111 k utterances/s at 128 x 8 s; a fifth: 97 k).
        The consumer's current stream waits for a result before it is yielded; the result stays valid until the consumer drops it."""
        if self.device.type != 'cuda':
            raise RuntimeError("nele_gan_amd: the enhancement path runs on the GPU only (no CPU fallback)")
        inflight = max(1, int(inflight))
        caller = torch.cuda.current_stream(self.device)
        n_side = inflight if inflight <= 3 else inflight - 1
        if len(self._slots) < n_side:
            # a hardware queue each for the first three (which of a process's streams share one is decided at their creation: two slots
            # on one queue run their batches one after the other - 65 k instead of 100 k utterances/s)
            if min(n_side, 3) > len(self._slots):
                # (round 6: and none of them on the CALLER's queue - "the default stream has a queue of its own" only holds in a fresh
                #  process; after a trainer has created its side streams a new stream may land on it: 93 k instead of 112 k with four in flight)
                self._slots += ops.streams_on_distinct_queues(self.device, min(n_side, 3) - len(self._slots), have=[caller] + self._slots)
            while len(self._slots) < n_side:
                self._slots.append(ops.side_stream(self.device))
        # the runtime has four hardware queues: the three side streams above + the one of the caller's own stream.  A FOURTH batch in
        # flight therefore runs on the caller's stream (a fourth side stream would share a queue with one of the three: 66 k utterances/s)
        slots = list(self._slots[:min(n_side, 3)]) + ([caller] if inflight >= 4 else []) + list(self._slots[3:n_side])
        G = self.G
        slot0 = G.buffer_slot
        was_frozen = G._weights_frozen and self._own_G and self._frozen_precision == G.precision
        frozen = G.freeze_weights(self.device)
        self._frozen_precision = G.precision
        pending = collections.deque()

        def hand_out():
            out, done, st = pending.popleft()
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(done)
            out.record_stream(cur)
            return out

        try:
            for k, batch in enumerate(batches):
                if len(pending) >= inflight:
                    yield hand_out()
                clean_wav, noise_wav = batch[0], batch[1]
                lengths = batch[2] if len(batch) > 2 else None
                st = slots[k % inflight]
                ready = torch.cuda.Event()
                ready.record(torch.cuda.current_stream(self.device))       # the inputs (and, first round, the frozen layouts) exist
                G.buffer_slot = ('stream', k % inflight)
                with torch.cuda.stream(st):
                    st.wait_event(ready)
                    if k < inflight:
                        st.wait_event(frozen)
                    out = self._enhance_impl(clean_wav, noise_wav, pcm16, lengths)
                    done = torch.cuda.Event()
                    done.record(st)
                for t in (clean_wav, noise_wav):
                    if t.is_cuda:
                        t.record_stream(st)
                pending.append((out, done, st))
            while pending:
                yield hand_out()
        finally:
            G.buffer_slot = slot0
            if not (self._own_G or was_frozen):
                G.unfreeze_weights()
            for _, done, _ in pending:                                   # a consumer that stopped early: nothing may still write when we return
                done.synchronize()


def enhance_files(enhancer, file_list, noise_path, output_path, batch=32, epoch_tag=1, sort_by_length=True, inflight=3, workers=8,
                  pad_to=4096, ahead=2, write=True):
    """inference.py:79-117 over ``file_list`` (clean wav paths; the noise file of each has the same name under ``noise_path``).
    Returns the list of written files ('<output_path>/<stem>@<epoch_tag>.wav'), in list order, for this rank's shard.

    Host side (the reference: one file at a time, librosa.load + sf.write in the main process): dataio.FileBatches reads a batch per
    library call (``workers`` library threads) straight into pinned int16 staging rows (batches padded to a multiple of ``pad_to``
    samples: few distinct shapes, the generator's buffers are cached per shape), uploads asynchronously, two batches ahead, and
    converts to float32 on the device;
    ``inflight`` batches are on the GPU at a time (enhance_stream); results are converted to their int16 sample values on the device, come
    back through pinned buffers on a copy stream and are written a batch per call by the library's own threads (nele_wav_write_pcm16_batch)
    while later batches run.  The host moves bytes only: no sample is touched by the interpreter or converted on a CPU core."""
    import concurrent.futures as cf
    import numpy as np
    from . import dataio
    dataio.creatdir(output_path)
    lo, hi = ndist.shard_range(len(file_list))                      # contiguous shard per rank; the whole list on one GPU
    mine = list(range(lo, hi))
    order = mine
    if sort_by_length:
        # batches of similar lengths waste less padding; the output list keeps the caller's order
        sizes = {i: os.path.getsize(file_list[i]) for i in mine}
        order = sorted(mine, key=lambda i: sizes[i])
    dev = enhancer.device
    fb = dataio.FileBatches([file_list[i] for i in order], noise_path, batch=batch, workers=workers, ahead=ahead, device=dev, pad_to=pad_to,
                            keep=inflight + ahead)
    if sort_by_length:
        for i in mine:                                                   # the sizes are known already: no second stat() per clean file
            fb._bounds[file_list[i]] = max(1, (sizes[i] - 44 + 1) // 2)
    written = {}
    names = {i: file_list[i].split('/')[-1] for i in mine}
    copy_out = torch.cuda.Stream(device=dev)
    pool = cf.ThreadPoolExecutor(max_workers=inflight + 2)           # a task = one batch's write call
    meta, outq, writes = [], collections.deque(), []

    def batches():
        for g in range(len(fb)):
            b = fb[g]
            meta.append((order[g * batch:(g + 1) * batch], b['lengths_host']))
            yield b['clean'], b['noise'], b['lengths']

    def flush(block_all):
        while outq and (block_all or outq[0][1].query()):
            host, ev, sel, lens = outq.popleft()
            ev.synchronize()
            paths = []
            for i in sel:
                path = dataio.enhanced_name(output_path, names[i], epoch_tag)
                paths.append(path)
                written[i] = path
            ns = [256 * (int(n) // 256) for n in lens]
            # one task per batch: the library's own threads write the files (nele_wav_write_pcm16_batch), no per-file work in the interpreter
            if write:
                writes.append((pool.submit(dataio.write_wav_batch_pcm16, paths, host.numpy(), ns, fs, workers), host))
            else:                                                        # (diagnostic: everything but the file writes)
                dataio.pinned_put(host)
        while writes and (block_all or writes[0][0].done()):
            fut, host = writes.pop(0)
            fut.result()                                                 # re-raises a writer's error
            dataio.pinned_put(host)                                     # the pinned buffer goes back to the pool

    try:
        for g, enh in enumerate(enhancer.enhance_stream(batches(), inflight=inflight, pcm16=True)):
            sel, lens = meta[g]
            meta[g] = None
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(dev))
            with torch.cuda.stream(copy_out):
                copy_out.wait_event(done)
                # the PCM_16 emulation left values k / 32768: k itself goes to the host (half the bytes), the writer threads add headers
                q = torch.empty(tuple(enh.shape), dtype=torch.int16, device=enh.device)
                _lib.check(_lib.lib.nele_float_to_pcm16(enh.data_ptr(), enh.shape[1], enh.shape[0], enh.shape[1], q.data_ptr(), enh.shape[1], 1,
                                                        copy_out.cuda_stream), 'nele_float_to_pcm16')
                enh.record_stream(copy_out)
                host = dataio.pinned_get(q.shape, torch.int16)
                host.copy_(q, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(copy_out)
            outq.append((host, ev, sel, lens))
            flush(False)
        flush(True)
    finally:
        pool.shutdown(wait=True)
        fb.close()
    return [written[i] for i in mine]


def score_enhanced(clean_path, noise_path, enhanced_names, groups=('Cafeteria', 'AirportAnnouncement'), quality=None, out=None):
    """inference.py:119-146: the true (unmapped) scores of the enhanced test files, per noise type - ``groups``: substrings of the file
    names (the reference's test set carries the noise type in the name); ``None`` / an empty tuple scores the whole list as one group ''.
    SIIB, HASPI and ESTOI through dataio.read_batch_* (one launch per metric and 256 files); PESQ and ViSQOL - external host programs,
    quality.py - when ``quality`` is true (None: when both programs are registered), else reported as nan.
    -> {group: {'siib', 'haspi', 'estoi', 'pesq', 'visqol': mean, 'files': n}}; the reference's report lines are printed to ``out``
    (a file object; default sys.stdout)."""
    import sys
    import numpy as np
    from . import dataio
    from . import quality as q
    if quality is None:
        quality = q._BACKENDS['visqol'] is not None and (q._BACKENDS['pesq'] is not None or q._BACKENDS['pesq_batch'] is not None)
    out = sys.stdout if out is None else out
    res = {}
    for g in (tuple(groups) if groups else ('',)):
        names = [x for x in enhanced_names if g in x]                               # :120
        if not names:
            continue
        r = {'haspi': float(np.mean(dataio.read_batch_HASPI(clean_path, noise_path, names, norm=False))),      # :122-131
             'estoi': float(np.mean(dataio.read_batch_STOI(clean_path, noise_path, names, norm=False))),
             'siib': float(np.mean(dataio.read_batch_SIIB(clean_path, noise_path, names, norm=False))),
             'pesq': float('nan'), 'visqol': float('nan'), 'files': len(names)}
        if quality:                                                                  # :134-141
            r['pesq'] = float(np.mean(q.read_batch_PESQ(clean_path, names, norm=False)))
            r['visqol'] = float(np.mean(q.read_batch_VISQOL(clean_path, names, norm=False)))
        res[g] = r
        out.write(g + ':\n')                                                         # :142-145
        out.write('SIIB is %.3f, HASPI is %.3f, ESTOI is %.3f, PESQ is %.3f, VISQOL is %.3f\n\n' % (r['siib'], r['haspi'], r['estoi'], r['pesq'], r['visqol']))
        out.write('======\n')
    return res


def score_quality(clean_path, enhanced_names, groups=('Cafeteria', 'AirportAnnouncement'), batch=32, out=None):
    """HASQI v2 (pyhaspi2.py:32-74) of (clean file, enhanced file) per noise group, both cut to the shorter one (what the reference's
    PESQ / ViSQOL calls compare: no listener's noise): metrics.batch_hasqi over batches of ``batch`` files, with the reference's
    basilar-membrane noise drawn per file (position in ``enhanced_names``).  The quality figure this build has without the two external
    programs, and what a D_Qua trained with ``--quality-targets hasqi`` predicts two terms of.
    -> {group: {'hasqi', 'nonlin', 'linear': mean over the files with a defined score, 'files': n}}; one report line per group."""
    import sys
    import numpy as np
    import torch
    from . import dataio
    from . import metrics as mt
    out = sys.stdout if out is None else out
    res = {}
    for g in (tuple(groups) if groups else ('',)):
        names = [(i, x) for i, x in enumerate(enhanced_names) if g in x]
        if not names:
            continue
        rows = []
        for k in range(0, len(names), batch):
            pairs = []
            for _i, f in names[k:k + batch]:
                c, e = dataio.load(clean_path + dataio.wave_name_of(f) + '.wav', sr=16000)[0], dataio.load(f, sr=16000)[0]
                n = min(len(c), len(e))
                pairs.append((c[:n], e[:n]))
            (c, lens), (e, _) = (dataio.pad_batch([p_[j] for p_ in pairs]) for j in range(2))
            rows.append(mt.batch_hasqi(c, e, 16000, lengths=torch.from_numpy(lens), noise='utterance', seed=0,
                                       utt_ids=[i for i, _f in names[k:k + batch]])[:, :3].cpu().numpy())
        rows = np.concatenate(rows)
        ok = rows[~np.isnan(rows[:, 0])]
        m = ok.mean(axis=0) if len(ok) else np.full(3, np.nan)
        res[g] = {'hasqi': float(m[0]), 'nonlin': float(m[1]), 'linear': float(m[2]), 'files': int(len(ok))}
        out.write('%s:\nHASQI is %.3f, Nonlin is %.3f, Linear is %.3f\n\n======\n' % (g, m[0], m[1], m[2]))
    return res


def score_rooms(clean_path, noise_path, enhanced_names, bank, batch=32, metrics=('siib', 'haspi', 'estoi'), out=None):
    """The scores of the enhanced files in the room each file's name gives (room.RirBank.ids: '<utt>#<rir>#...wav'; no such RIR:
    anechoic), eval_metrics.py:100-186 per utterance: eval_metrics.evaluate_rooms over batches of ``batch`` files.
    -> {rir name (None = anechoic): {metric: mean, 'files': n}}; one report line per RIR is printed to ``out``."""
    import sys
    import numpy as np
    from . import dataio, eval_metrics
    out = sys.stdout if out is None else out
    ids = bank.ids([dataio.wave_name_of(f) + '.wav' for f in enhanced_names])
    rows = {m: [] for m in metrics}
    for k in range(0, len(enhanced_names), batch):
        trip = []
        for f in enhanced_names[k:k + batch]:
            name = dataio.wave_name_of(f) + '.wav'
            c, e, v = dataio.load(clean_path + name, sr=16000)[0], dataio.load(f, sr=16000)[0], dataio.load(noise_path + name, sr=16000)[0]
            n = min(len(c), len(e), len(v))                                          # eval_metrics.py:111-114
            trip.append((c[:n], e[:n], v[:n]))
        (c, lens), (e, _), (v, _) = (dataio.pad_batch([t[i] for t in trip]) for i in range(3))
        r = eval_metrics.evaluate_rooms(c, e, v, bank, ids[k:k + batch], lengths=lens, metrics=metrics)
        for m in metrics:
            rows[m].append(r[m])
    rows = {m: np.concatenate(v) for m, v in rows.items()}
    res = {}
    for i in sorted(set(ids.tolist())):
        name = bank.name_of(i)
        res[name] = {m: float(np.mean(rows[m][ids == i])) for m in metrics}
        res[name]['files'] = int((ids == i).sum())
        out.write('%s:\n%s\n\n======\n' % ('NO_rev' if name is None else name, ', '.join('%s is %.3f' % (m.upper(), res[name][m]) for m in metrics)))
    return res


BASELINES = ('clean', 'ssdrc', 'siiopt')


def baseline_files(tag, clean_files, work_dir, batch=32, noise_path=None):
    """The files a baseline is scored from, named like the clean files: 'clean' - the unprocessed speech itself; 'ssdrc' - SSDRC of every
    clean file (ssdrc.py), written as PCM_16 under ``work_dir/baseline_ssdrc/MultiEnh/`` like every enhanced file that is scored;
    'siiopt' - the SII-optimal rule (siiopt.py) on every clean file against its noise file under ``noise_path``, likewise under
    ``work_dir/baseline_siiopt/MultiEnh/``."""
    import os
    if tag == 'clean':
        return list(clean_files)
    if tag == 'siiopt':
        if noise_path is None:
            raise ValueError("baseline 'siiopt' adapts to the noise: it needs noise_path")
        from . import siiopt as _siiopt
        root = os.path.join(work_dir, 'baseline_siiopt')
        _siiopt.siiopt_corpus(clean_files, noise_path, root, batch=batch)
        return [os.path.join(root, 'MultiEnh', f.split('/')[-1]) for f in clean_files]
    if tag != 'ssdrc':
        raise ValueError("baseline must be one of %s" % (BASELINES,))
    from . import ssdrc as _ssdrc
    root = os.path.join(work_dir, 'baseline_ssdrc')
    _ssdrc.ssdrc_corpus(clean_files, root, batch=batch)
    return [os.path.join(root, 'MultiEnh', f.split('/')[-1]) for f in clean_files]


def score_baseline(tag, clean_path, noise_path, clean_files, work_dir, groups=('Cafeteria', 'AirportAnnouncement'), bank=None, batch=32, quality=None,
                   out=None):
    """eval_metrics.py:107-108: a baseline (``tag``: 'clean', 'ssdrc' or 'siiopt') through the very path the generator's files take - score_enhanced
    per noise group and, with ``bank``, score_rooms per RIR.  -> (score_enhanced's dict, score_rooms' dict or None)."""
    import sys
    out = sys.stdout if out is None else out
    names = baseline_files(tag, clean_files, work_dir, batch=batch, noise_path=noise_path)
    out.write('baseline %s\n' % tag)
    res = score_enhanced(clean_path, noise_path, names, groups=groups, quality=quality, out=out)
    rooms = score_rooms(clean_path, noise_path, names, bank, batch=batch, out=out) if bank is not None else None
    return res, rooms


def main(argv=None):
    """``python -m nele_gan_amd.inference --chkpt ./trained_model/chkpt_GD.pt --clean <dir> --noise <dir> --output <dir>`` = the
    reference's usage step 4 (`python inference.py`, README; inference.py:28-146): every wav under --clean is enhanced against the noise file
    of the same name, written as '<output>/<name>@1.wav' (PCM_16), and - ``--score`` - the per-noise report of :119-146 is printed."""
    import argparse
    from . import dataio
    ap = argparse.ArgumentParser(prog='python -m nele_gan_amd.inference', description=main.__doc__)
    ap.add_argument('--chkpt', default=None, help="checkpoint with an 'enhance-model' entry (reference checkpoints load unchanged); default: random weights")
    ap.add_argument('--rule', choices=('siiopt',), default=None, help="instead of --chkpt: a training-free rule in the generator's place - 'siiopt', SII-optimal band gains "
                                                                      "on the noise estimate (no checkpoint needed)")
    ap.add_argument('--rule-strength', type=float, default=0.5, help='with --rule siiopt: exponent on the optimal gain, in (0, 1]')
    ap.add_argument('--clean', required=True)
    ap.add_argument('--noise', required=True)
    ap.add_argument('--output', default='./output_inference')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--precision', choices=('bf16', 'bf16x3', 'f32'), default='bf16')
    ap.add_argument('--norm', choices=M.NORMS, default=None, help="energy normalisation (default: what the checkpoint records, else 'utterance'); 'prefix' = the causal form the real-time path emits")
    ap.add_argument('--score', action='store_true', help='SIIB / HASPI / ESTOI (PESQ / ViSQOL when registered) of the written files')
    ap.add_argument('--score-quality', action='store_true', help='with --score: also HASQI v2 Combined / Nonlin / Linear of (clean, enhanced), computed on the GPU '
                                                                 '(no external program)')
    ap.add_argument('--groups', default='Cafeteria,AirportAnnouncement', help='noise types (substrings of the file names) reported separately; empty = all files together')
    ap.add_argument('--rir', default=None, help="with --score: folder of 16 kHz room impulse responses; the files are also scored in the room their name gives "
                                                "('<utt>#<rir>#...wav'), reported per RIR")
    ap.add_argument('--baseline', action='append', choices=BASELINES, default=None,
                    help="with --score: also score a baseline beside the generator - 'ssdrc' (SSDRC of the clean files), 'siiopt' (SII-optimal band gains against the noise "
                         "files) or 'clean' (the unprocessed speech); may repeat")
    from . import roomsynth as _rs
    _rs.add_cli_arguments(ap)
    from . import quality as _q
    _q.add_cli_arguments(ap)
    a = ap.parse_args(argv)
    if a.rooms_synth and not a.score:
        ap.error('--rooms-synth needs --score')
    if a.baseline and not a.score:
        ap.error('--baseline needs --score')
    if a.score_quality and not a.score:
        ap.error('--score-quality needs --score')
    if a.rule and a.chkpt:
        ap.error('--rule takes the place of --chkpt; pass one of them')
    _q.backends_from_cli(a)
    if a.rule:
        from . import siiopt as _siiopt
        try:
            e = Enhancer(G=_siiopt.SiiOptRule(a.rule_strength), norm=a.norm)
        except ValueError as err:
            ap.error(str(err))
    else:
        e = Enhancer(a.chkpt, norm=a.norm)
        e.G.precision = a.precision
    files = sorted(dataio.get_filepaths(a.clean))
    noise = a.noise.rstrip('/') + '/'
    out = enhance_files(e, files, noise, a.output, batch=a.batch)
    print('%d files -> %s' % (len(out), a.output))
    if a.score:
        groups = tuple(g for g in a.groups.split(',') if g)
        bank = None
        score_enhanced(a.clean.rstrip('/') + '/', noise, out, groups=groups)
        if a.score_quality:
            score_quality(a.clean.rstrip('/') + '/', out, groups=groups, batch=a.batch)
        if a.rooms_synth:
            bank = _rs.bank_from_cli(ap, a)                              # (refuses --rir beside it)
        elif a.rir:
            from . import room
            bank = room.RirBank(a.rir)
        if bank is not None:
            score_rooms(a.clean.rstrip('/') + '/', noise, out, bank, batch=a.batch)
        for tag in a.baseline or ():
            score_baseline(tag, a.clean.rstrip('/') + '/', noise, files, a.output, groups=groups, bank=bank, batch=a.batch)
    return 0


if __name__ == '__main__':
    import sys
    sys.exit(main())
