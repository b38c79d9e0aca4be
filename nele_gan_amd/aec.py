"""Acoustic echo cancellation for the real-time enhancer: the microphone at the listener's end hears the room's noise AND the loudspeaker
playing the enhancer's own output; ``EchoCanceller`` takes the loudspeaker's part out of it, so that what reaches ``RealtimeEnhancer`` as
`noise` is the noise.  One partitioned-block frequency-domain adaptive filter per stream slot (256-sample hops, 512-point float64
transforms, P partitions = 256 P samples of echo tail) in libnele_hip.so (csrc/aec.hip, the ``nele_aec_*`` entry points; the arithmetic
is DESIGN.md section 14).  This module owns memory and bookkeeping only; there is no arithmetic in torch.

    aec = EchoCanceller(streams=256, partitions=8)
    residual = aec.process(mic_hops, played_hops)              # [256, nh * 256] each -> mic minus the estimated echo of `played`
    h = aec.echo_path()                                        # [256, 8 * 256] float64: the impulse responses estimated so far

    loop = EchoCancellingEnhancer(RealtimeEnhancer(...), aec)  # closes the loop: what process() returns is what the loudspeaker plays
    out = loop.process(clean_hops, mic_hops)                   # during the next call's capture

    python -m nele_gan_amd.aec --mic mic.wav --played far.wav --out residual.wav [--partitions 8] [--echo-path h.npy] [--bulk-blocks 32 [--bulk-track]
                               [--drift [--drift-ppm PPM]]] [--suppress [--res-beta 2.0] [--res-gmin 0.1]]
                               [--uplink uplink.wav [--uplink-gmin 0.1]]

A bulk delay (the device's playback and capture buffers) is found and taken out ahead of the canceller by nele_gan_amd/bulkdelay.py
(``AlignedEchoCanceller``; --bulk-blocks on the command line), and followed when it moves later by nele_gan_amd/bulktrack.py
(``TrackedEchoCanceller``; --bulk-track); clock drift between playback and capture is followed by nele_gan_amd/drift.py
(``DriftTrackedEchoCanceller``; --drift).  The echo the canceller leaves is suppressed behind it by
nele_gan_amd/res.py (``SuppressedEchoCanceller``; --suppress on the command line).  The near-end noise in the residual is suppressed for
the uplink by nele_gan_amd/ns.py (``NoiseSuppressor``; --uplink).
"""
import numpy as np
import torch

from . import _lib
from ._lib import c_longlong, call, ptr, stream
from ._slots import SlotState, dev_rows, to_dev

HOP = 256
MAX_PARTITIONS = _lib.CONSTS['NELE_AEC_MAX_PARTITIONS']


class EchoCanceller(SlotState):
    """B independent echo cancellers.  partitions: P in 1 .. 32, the echo tail the filter covers is 256 P samples (128 ms at P = 8);
    mu (0 < mu < 2), gamma (>= 0), delta (> 0): the step of DESIGN.md section 14 - the weights move by
    mu E conj(X_p) / (sum_p |X_p|^2 + gamma P S_e + delta), S_e the smoothed power of the residual."""

    def __init__(self, streams, partitions=8, mu=0.5, gamma=4.0, delta=1e-2, device='cuda'):
        super().__init__(streams)
        self.P = int(partitions)
        if not 1 <= self.P <= MAX_PARTITIONS:
            raise ValueError("EchoCanceller: partitions must be in 1 .. %d (got %d)" % (MAX_PARTITIONS, self.P))
        self.mu, self.gamma, self.delta = float(mu), float(gamma), float(delta)
        if not (0.0 < self.mu < 2.0) or not (self.gamma >= 0.0) or not (self.delta > 0.0):
            raise ValueError("EchoCanceller: needs 0 < mu < 2, gamma >= 0 and delta > 0 (got %g, %g, %g)" % (self.mu, self.gamma, self.delta))
        self._alloc(device, _lib.lib.nele_aec_state_bytes(self.S, self.P))
        call('nele_aec_init', ptr(self.state), c_longlong(self.nbytes), self.S, self.P, stream())

    # ---- streaming
    def process(self, mic, played, active=None, adapt=None, want_echo=False, out=None):
        """mic, played [streams, nh * 256] float32 (host, pinned host or device) -> residual [streams, nh * 256] on the device: mic minus
        the echo of `played` as estimated so far (with want_echo: (residual, echo)).  played: what the loudspeaker put out while mic was
        captured, hop for hop; a constant extra delay is part of the echo path.  active / adapt: host bool sequences [streams] or None
        (all): inactive slots are neither read nor changed and their output columns are left as they were; slots with adapt false
        cancel with the filter they have and do not move it.  out (beyond RealtimeEnhancer's signature): a residual buffer, or
        (residual, echo), on the device to write into - the way to keep an inactive slot's columns; without it the outputs are fresh
        tensors and an inactive slot's columns undefined.  Never blocks the host."""
        res, echo = (out if isinstance(out, (tuple, list)) else (out, None)) if out is not None else (None, None)
        shape, nh, d, x, act, flags, res = self._hop_args(mic, played, ('mic', 'played'), active, res, what='out buffers')
        ada = None if adapt is None else self._dev_bytes(self._flags(adapt, "EchoCanceller: adapt must hold one flag per stream"))
        echo = self._out(echo, shape, what='out buffers') if want_echo else None
        call('nele_aec_hop', ptr(self.state), c_longlong(self.nbytes), self.S, self.P, ptr(d), ptr(x), ptr(flags), ptr(ada), nh, self.mu, self.gamma,
             self.delta, ptr(res), ptr(echo), stream())
        self._count(act, nh)
        return (res, echo) if want_echo else res

    def echo_path(self, slots=None):
        """-> float64 [len(slots), partitions * 256] on the device (all slots when None): h[256 p + n] = irfft512(W_p)[n], the impulse
        response from `played` to `mic` as estimated so far (zeros after a reset)."""
        h = torch.empty((self.S, self.P * HOP), dtype=torch.float64, device=self.device)
        call('nele_aec_echo_path', ptr(self.state), c_longlong(self.nbytes), self.S, self.P, ptr(h), stream())
        if slots is None:
            return h
        return h.index_select(0, self._dev_rows(slots))

    def reset(self, slots):
        """Restart the given slots (zero weights, history and S_e); the other slots are not touched."""
        m = self._slots_mask(slots)
        call('nele_aec_reset', ptr(self.state), c_longlong(self.nbytes), self.S, self.P, ptr(self._dev_bytes(m)), stream())
        self.hops[m] = 0

    def reset_flagged(self, flags):
        """reset() of the slots with flags[b] != 0, flags a uint8 [streams] tensor ON THE DEVICE (bulktrack.TrackingBulkDelay's `moved`):
        which slots restart is decided on the GPU, the host neither reads the flags nor waits - and so its counter ``hops`` is not
        told."""
        if tuple(flags.shape) != (self.S,) or flags.dtype != torch.uint8:
            raise ValueError("EchoCanceller.reset_flagged: flags must be uint8 [%d] on the device" % self.S)
        call('nele_aec_reset', ptr(self.state), c_longlong(self.nbytes), self.S, self.P, ptr(flags), stream())


class EchoCancellingEnhancer:
    """``RealtimeEnhancer`` behind an ``EchoCanceller``, the loop closed: per call
        residual = aec.process(mic, played);  out = rt.process(clean, residual);  played <- out (active slots)
    with played = zeros before a slot's first call and after its reset.  The caller's promise: what process() returns is what the
    loudspeaker plays during the NEXT call's capture (any constant extra delay is part of the echo path the canceller learns).  The
    number of hops per call is fixed by the first call."""

    def __init__(self, rt, aec):
        if rt.S != aec.S:
            raise ValueError("EchoCancellingEnhancer: the enhancer has %d streams, the canceller %d" % (rt.S, aec.S))
        self.rt, self.aec, self.S = rt, aec, rt.S
        self.played = None                                 # [S, nh * 256] on the canceller's device, from the first call on

    def _played(self, width):
        if self.played is None:
            self.played = torch.zeros((self.S, width), dtype=torch.float32, device=self.aec.device)
        elif self.played.shape[1] != width:
            raise ValueError("EchoCancellingEnhancer: %d hops per call, this call brings %d (fixed for the object's life)"
                             % (self.played.shape[1] // HOP, width // HOP))
        return self.played

    def process(self, clean, mic, active=None, debug=None, want_residual=False):
        """clean, mic [streams, nh * 256] float32 -> out [streams, nh * 256] (RealtimeEnhancer.process on the echo-cancelled mic).
        The returned tensor is the caller's: the loop keeps its own copy of what was played.  debug: RealtimeEnhancer's RealtimeDebug.
        want_residual: -> (out, residual), the canceller's residual of this call as the enhancer read it - the near-end signal, what
        the uplink carries (nele_gan_amd/ns.py's DuplexEnhancer suppresses its noise)."""
        shape = tuple(np.shape(mic))
        if len(shape) != 2 or shape[1] % HOP or shape[1] == 0:
            raise ValueError("EchoCancellingEnhancer.process: mic must be [%d, nh * 256]" % self.S)
        played = self._played(shape[1])
        residual = self.aec.process(mic, played, active=active)
        out = self.rt.process(clean, residual, active=active) if debug is None else self.rt.process(clean, residual, active=active, debug=debug)
        if active is None:
            played.copy_(out)                              # an owned buffer: later calls and reset() change it in place
        else:
            rows = dev_rows(np.nonzero(np.asarray(active, dtype=bool).reshape(-1))[0], played.device)
            played.index_copy_(0, rows, out.index_select(0, rows))
        return (out, residual) if want_residual else out

    def finish(self, slots, clean_tail, mic_tail, tail_lengths, debug=None):
        """End the streams of ``slots`` (RealtimeEnhancer.finish): the tails [len(slots), <= 256] are padded to one hop, one canceller hop
        runs on those slots (against the first hop of what they were last given to play) and the first tail_lengths[i] samples of its
        residual are the noise tails of rt.finish."""
        slots = np.asarray(slots, dtype=np.int64).reshape(-1)
        mt = torch.as_tensor(mic_tail, dtype=torch.float32).reshape(len(slots), -1)
        if mt.shape[1] > HOP:
            raise ValueError("EchoCancellingEnhancer.finish: tails must be [len(slots), <= 256]")
        played = self._played(HOP if self.played is None else self.played.shape[1])
        rows = dev_rows(slots, played.device)
        mic = torch.zeros((self.S, HOP), dtype=torch.float32, device=played.device)
        mic[:, :mt.shape[1]].index_copy_(0, rows, to_dev(mt, played.device))
        act = np.zeros(self.S, dtype=bool)
        act[slots] = True
        residual = self.aec.process(mic, played[:, :HOP].contiguous(), active=act)
        ct = torch.as_tensor(clean_tail, dtype=torch.float32).reshape(len(slots), -1)
        if ct.shape[1] < HOP:
            ct = torch.nn.functional.pad(ct, (0, HOP - ct.shape[1]))
        kw = {} if debug is None else {'debug': debug}
        return self.rt.finish(slots, to_dev(ct, played.device), residual.index_select(0, rows), tail_lengths, **kw)

    def reset(self, slots):
        """Restart the given slots in both objects; they play zeros until their next call."""
        self.rt.reset(slots)
        self.aec.reset(slots)
        if self.played is not None:
            self.played.index_fill_(0, dev_rows(slots, self.played.device), 0.0)


# ------------------------------------------------------------------------------------------------------------------ command line
def _cancel_file_drift(d, x, L, aec, partitions, device, bulk_blocks, suppress, bulk_track, drift_ppm):
    """cancel_file with drift: search, drift.DriftCompensator and canceller (drift.DriftTrackedEchoCanceller), hop by hop"""
    from .bulkdelay import BulkDelay
    from .bulktrack import TrackingBulkDelay
    from .drift import DriftCompensator, DriftTrackedEchoCanceller
    bulk = (TrackingBulkDelay if bulk_track else BulkDelay)(1, blocks=bulk_blocks, device=device)
    comp = DriftCompensator(1, blocks=bulk_blocks, device=device)
    if drift_ppm:
        comp.set_rate([0], drift_ppm)
    chain = DriftTrackedEchoCanceller(bulk, comp, aec)
    if suppress is not None:
        from .res import ResidualEchoSuppressor, SuppressedEchoCanceller
        chain = SuppressedEchoCanceller(chain, ResidualEchoSuppressor(1, beta=suppress[0], gmin=suppress[1], device=device))
    dd, xd = to_dev(torch.from_numpy(d), bulk.device), to_dev(torch.from_numpy(x), bulk.device)
    res, events, last = [], [], -1
    for k in range(d.shape[1] // HOP):
        res.append(chain.process(dd[:, k * HOP:(k + 1) * HOP].contiguous(), xd[:, k * HOP:(k + 1) * HOP].contiguous()))
        if bulk_track:
            now = int(bulk.delays()[0].item())
            if now != last:
                events.append((k, now))
                last = now
    found = events if bulk_track else int(bulk.delays()[0].item())
    return torch.cat(res, dim=1)[0, :L].cpu().numpy(), chain.echo_path()[0].cpu().numpy(), found, float(comp.status()['drift_ppm'][0].item())


def cancel_file(mic, played, partitions=8, mu=0.5, gamma=4.0, delta=1e-2, device='cuda', bulk_blocks=None, suppress=None, bulk_track=False,
                drift=False, drift_ppm=0.0):
    """mic, played: float32 arrays of one length L -> (residual [L] float32, echo path [partitions * 256] float64): the whole hops through
    one EchoCanceller call, the last L % 256 samples zero-padded to one more hop and cut again.  bulk_blocks: search that many blocks
    for a bulk delay and cancel against `played` delayed by it (bulkdelay.AlignedEchoCanceller); the return value gains a third
    element, the delay found in hops (-1: none).  bulk_track (with bulk_blocks): the search goes on behind the lock and follows the delay
    when it moves (bulktrack.TrackedEchoCanceller); the file then goes through hop by hop, the delay is read back after every hop, and
    the third element is the list of (hop, delay in hops) of the lock and of every move (empty: none found).  suppress: (beta, gmin)
    of a res.ResidualEchoSuppressor behind the canceller (res.SuppressedEchoCanceller): the residual is the suppressed one, one hop late as process() returns it - its first 256 samples
    are the canceller's own residual and the file's last hop does not come out.  drift (with bulk_blocks): a drift.DriftCompensator
    between the search and the canceller follows the clock drift between `played` and `mic` (drift.DriftTrackedEchoCanceller); the file
    goes through hop by hop and the return value gains a fourth element, the final drift estimate in ppm; drift_ppm: the estimate
    it starts from."""
    mic = np.ascontiguousarray(mic, dtype=np.float32).reshape(-1)
    played = np.ascontiguousarray(played, dtype=np.float32).reshape(-1)
    if mic.shape != played.shape or mic.size == 0:
        raise ValueError("aec: --mic and --played must have one length (got %d and %d samples)" % (mic.size, played.size))
    if drift and bulk_blocks is None:
        raise ValueError("aec: drift needs bulk_blocks: the compensator stands on the whole-hop delay the search finds")
    L = mic.size
    nh = (L + HOP - 1) // HOP
    d = np.zeros((1, nh * HOP), dtype=np.float32)
    x = np.zeros((1, nh * HOP), dtype=np.float32)
    d[0, :L], x[0, :L] = mic, played
    aec = EchoCanceller(1, partitions=partitions, mu=mu, gamma=gamma, delta=delta, device=device)
    if drift:
        return _cancel_file_drift(d, x, L, aec, partitions, device, bulk_blocks, suppress, bulk_track, drift_ppm)
    if bulk_blocks is not None and bulk_track:
        from .bulktrack import TrackedEchoCanceller, TrackingBulkDelay
        bulk = TrackingBulkDelay(1, blocks=bulk_blocks, device=device)
        aec = TrackedEchoCanceller(bulk, aec)
    elif bulk_blocks is not None:
        from .bulkdelay import AlignedEchoCanceller, BulkDelay
        bulk = BulkDelay(1, blocks=bulk_blocks, device=device)
        aec = AlignedEchoCanceller(bulk, aec)
    if suppress is not None:
        from .res import ResidualEchoSuppressor, SuppressedEchoCanceller
        aec = SuppressedEchoCanceller(aec, ResidualEchoSuppressor(1, beta=suppress[0], gmin=suppress[1], device=device))
    if bulk_blocks is not None and bulk_track:
        dd, xd = to_dev(torch.from_numpy(d), bulk.device), to_dev(torch.from_numpy(x), bulk.device)
        res, events, last = [], [], -1
        for k in range(nh):
            res.append(aec.process(dd[:, k * HOP:(k + 1) * HOP].contiguous(), xd[:, k * HOP:(k + 1) * HOP].contiguous()))
            now = int(bulk.delays()[0].item())
            if now != last:
                events.append((k, now))
                last = now
        return torch.cat(res, dim=1)[0, :L].cpu().numpy(), aec.echo_path()[0].cpu().numpy(), events
    res = aec.process(torch.from_numpy(d), torch.from_numpy(x))
    h = aec.echo_path()
    if bulk_blocks is not None:
        return res[0, :L].cpu().numpy(), h[0].cpu().numpy(), int(bulk.delays()[0].item())
    return res[0, :L].cpu().numpy(), h[0].cpu().numpy()


def build_parser():
    import argparse
    ap = argparse.ArgumentParser(prog='python -m nele_gan_amd.aec', description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--mic', required=True, help='16 kHz PCM_16 wav: what the microphone captured')
    ap.add_argument('--played', required=True, help='16 kHz PCM_16 wav of the same length: what the loudspeaker played meanwhile')
    ap.add_argument('--out', required=True, help='the residual (mic minus the estimated echo), PCM_16')
    ap.add_argument('--partitions', type=int, default=8, help='256-sample blocks of echo tail the filter covers, 1 .. 32')
    ap.add_argument('--echo-path', default=None, metavar='NPY', help='write the final impulse-response estimate (float64 [partitions * 256])')
    ap.add_argument('--bulk-blocks', type=int, default=None, metavar='N',
                    help='search N 256-sample blocks (2 .. 64) for a bulk delay and cancel against --played delayed by the whole hops found '
                         '(default: no search)')
    ap.add_argument('--bulk-track', action='store_true',
                    help='with --bulk-blocks: go on searching behind the lock and follow the delay when it moves (nele_gan_amd/bulktrack.py)')
    ap.add_argument('--drift', action='store_true',
                    help='with --bulk-blocks: follow the clock drift between --played and --mic ahead of the canceller (nele_gan_amd/drift.py) '
                         'and print the final estimate')
    ap.add_argument('--drift-ppm', type=float, default=None, metavar='PPM',
                    help='with --drift: the estimate to start from, how fast the capture clock runs, within +-1000 (default 0)')
    ap.add_argument('--suppress', action='store_true',
                    help='suppress the echo the canceller leaves (nele_gan_amd/res.py); the output is then one 256-sample hop late')
    ap.add_argument('--res-beta', type=float, default=2.0, help='with --suppress: the over-subtraction factor, >= 0')
    ap.add_argument('--res-gmin', type=float, default=0.1, help='with --suppress: the floor of the gain, in (0, 1]')
    ap.add_argument('--uplink', default=None, metavar='WAV',
                    help='also write the residual with its noise suppressed (nele_gan_amd/ns.py), PCM_16: what the far end hears, one '
                         '256-sample hop later than --out')
    ap.add_argument('--uplink-gmin', type=float, default=None, metavar='G', help='with --uplink: the gain of a bin without speech, in (0, 1] (default 0.1)')
    ap.add_argument('--mu', type=float, default=0.5)
    ap.add_argument('--gamma', type=float, default=4.0)
    ap.add_argument('--delta', type=float, default=1e-2)
    return ap


def main(argv=None):
    from . import dataio
    ap = build_parser()
    a = ap.parse_args(argv)
    if not 1 <= a.partitions <= MAX_PARTITIONS:
        ap.error('--partitions must be in 1 .. %d' % MAX_PARTITIONS)
    if not (0.0 < a.mu < 2.0) or not (a.gamma >= 0.0) or not (a.delta > 0.0):
        ap.error('needs 0 < --mu < 2, --gamma >= 0 and --delta > 0')
    sig = []
    for path in (a.mic, a.played):
        wav, sr = dataio.read_wav(path)
        if sr != dataio.fs:
            ap.error('%s is sampled at %d Hz, not %d: convert it first with python -m nele_gan_amd.resample' % (path, sr, dataio.fs))
        sig.append(wav)
    if len(sig[0]) != len(sig[1]) or len(sig[0]) == 0:
        ap.error('--mic and --played must have one length (got %d and %d samples)' % (len(sig[0]), len(sig[1])))
    if a.bulk_blocks is not None and not 2 <= a.bulk_blocks <= _lib.CONSTS['NELE_BULK_MAX_BLOCKS']:
        ap.error('--bulk-blocks must be in 2 .. %d' % _lib.CONSTS['NELE_BULK_MAX_BLOCKS'])
    if a.suppress and (not (0.0 <= a.res_beta < float('inf')) or not (0.0 < a.res_gmin <= 1.0)):
        ap.error('needs --res-beta >= 0 and 0 < --res-gmin <= 1')
    if a.bulk_track and a.bulk_blocks is None:
        ap.error('--bulk-track needs --bulk-blocks')
    if a.drift and a.bulk_blocks is None:
        ap.error('--drift needs --bulk-blocks: the compensator stands on the whole-hop delay the search finds')
    if a.drift_ppm is not None and not a.drift:
        ap.error('--drift-ppm needs --drift (and --bulk-blocks)')
    if a.drift_ppm is not None and not abs(a.drift_ppm) <= 1000.0:
        ap.error('--drift-ppm must be within +-1000')
    if a.uplink_gmin is not None and a.uplink is None:
        ap.error('--uplink-gmin needs --uplink')
    if a.uplink_gmin is not None and not (0.0 < a.uplink_gmin <= 1.0):
        ap.error('needs 0 < --uplink-gmin <= 1')
    suppress = (a.res_beta, a.res_gmin) if a.suppress else None
    drift = {'drift': True, 'drift_ppm': a.drift_ppm or 0.0} if a.drift else {}
    res, h, *found = cancel_file(sig[0], sig[1], partitions=a.partitions, mu=a.mu, gamma=a.gamma, delta=a.delta, bulk_blocks=a.bulk_blocks,
                                 suppress=suppress, bulk_track=a.bulk_track, **drift)
    dataio.write_wav_pcm16(a.out, res)
    if a.uplink:
        from .ns import suppress_file
        gmin = 0.1 if a.uplink_gmin is None else a.uplink_gmin
        dataio.write_wav_pcm16(a.uplink, suppress_file(res, gmin=gmin))
        print('%s: the residual with its noise suppressed (gmin %g), one hop (%d ms) later than %s' % (a.uplink, gmin, HOP * 1000 // dataio.fs, a.out))
    if a.echo_path:
        np.save(a.echo_path, h)
    print('%s: %d samples, %d partitions (%d ms of echo tail)' % (a.out, len(res), a.partitions, a.partitions * HOP * 1000 // dataio.fs))
    if found and a.bulk_track:
        if not found[0]:
            print('bulk delay: none found in %d blocks' % a.bulk_blocks)
        for i, (k, hops) in enumerate(found[0]):
            print('bulk delay: %s at hop %d: %d hops (%d ms) taken out ahead of the canceller'
                  % ('moved' if i else 'locked', k, hops, hops * HOP * 1000 // dataio.fs))
    elif found:
        print('bulk delay: %s' % ('none found in %d blocks' % a.bulk_blocks if found[0] < 0 else
                                  '%d hops (%d ms) taken out ahead of the canceller' % (found[0], found[0] * HOP * 1000 // dataio.fs)))
    if a.drift:
        print('clock drift: %.1f ppm (how fast the capture clock runs against the playback clock) followed ahead of the canceller' % found[1])
    if a.suppress:
        print('residual echo suppressed (beta %g, gmin %g): the output is one hop (%d ms) late' % (a.res_beta, a.res_gmin, HOP * 1000 // dataio.fs))
    return 0


if __name__ == '__main__':
    import sys
    sys.exit(main())
