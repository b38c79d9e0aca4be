"""A running ESTOI per stream, so that the real-time loop can say what it gains: every other figure of the chain comes from offline
references on whole utterances.  ``StreamMonitor`` is the batch ESTOI of csrc/estoi.hip as a hop-by-hop stage with state, per stream
slot: ESTOI's own 16 -> 10 kHz filter, its frames, its 40 dB gate against the loudest frame SO FAR, the overlap-add and re-analysis of
the kept frames, a ring of the last 30 third-octave band vectors and one segment value d per new vector - in libnele_hip.so
(csrc/monitor.hip, the ``nele_mon_*`` entry points of include/nele_hip_ext10.h; the measure is DESIGN.md section 27).  The mean of d
over a stream is its ESTOI; on a signal whose loudest frame comes first it is the offline figure, segment for segment.  This module
owns memory and bookkeeping only; there is no arithmetic in torch but the readings' quotient and logistic map.

    mon = StreamMonitor(streams=256, lag=1)                     # out of a RealtimeEnhancer is one hop behind clean
    mon.process(clean_hops, out_hops, noise_hops)               # nothing returned, nothing read back; one launch
    r = mon.read()                                              # r.estoi, r.last, r.smoothed, r.segments, r.skipped: [256] on the device
    stats, seg, nseg = mon.process(clean_hops, out_hops, noise_hops, want=('stats', 'seg', 'nseg'))

    chain = MonitoredEnhancer(RealtimeEnhancer(rule=SiiOptRule(), streams=256), mon, baseline=StreamMonitor(256, lag=1))
    out = chain.process(clean_hops, noise_hops)                 # the inner object's output, bit for bit
    gain = chain.benefit()                                      # smoothed ESTOI of (out + noise) minus that of (clean + noise), [256]

    python -m nele_gan_amd.monitor --clean speech.wav --noise noise.wav [--chkpt G.pt | --rule siiopt] [--csv hops.csv]

The first ``lag`` hops of a slot only fill the history of ``ref``; nothing is measured in them.  A reading of a slot without a counted
segment has ``estoi`` NaN (0 / 0): about 0.4 s of kept frames pass before the first.
"""
import collections
import math

import numpy as np
import torch

from ._lib import CONSTS10, c_longlong, call, lib, ptr, stream
from ._slots import SlotState

HOP = CONSTS10['NELE_MON_HOP']
NSTATS = CONSTS10['NELE_MON_STATS']
MAX_LAG = CONSTS10['NELE_MON_MAX_LAG']
WANT = ('stats', 'seg', 'nseg')
SEGMENT_SECONDS = 0.0128                                    # one segment per kept frame: 128 samples at 10 kHz
COUNT, SUM, LAST, SMOOTH, SKIPPED, SEEN, KEPT, LOUDEST = range(8)

Reading = collections.namedtuple('Reading', 'stats estoi last smoothed segments skipped')


def smoothing_factor(time_constant):
    """a time constant in seconds -> the factor per counted segment, 1 - exp(-0.0128 / time_constant), which must lie in (0, 1]"""
    tc = float(time_constant)
    if not (tc > 0.0 and math.isfinite(tc)):
        raise ValueError("StreamMonitor: time_constant must be a positive number of seconds (got %r)" % (time_constant,))
    a = float(1.0 - np.exp(-SEGMENT_SECONDS / tc))
    if not 0.0 < a <= 1.0:
        raise ValueError("StreamMonitor: time_constant=%g s is too long: its factor per segment rounds to 0" % tc)
    return a


def map_estoi(d):
    """metrics.mapping_ESTOI_harvard on a tensor: 1 / (1 + exp(-8 (d - 0.25)))"""
    return 1 / (1 + torch.exp(-8.0 * (d - 0.25)))


class StreamMonitor(SlotState):
    """B independent running ESTOI measures.  lag: the hops, 0 .. 4, by which ``deg`` is behind ``ref`` (1 behind a RealtimeEnhancer, 2
    behind a CompressedEnhancer, a LimitedEnhancer's ``lag_hops``).  time_constant [s]: of the smoothed reading."""

    def __init__(self, streams, lag=1, time_constant=1.0, device='cuda'):
        super().__init__(streams)
        if isinstance(lag, bool) or int(lag) != lag or not 0 <= int(lag) <= MAX_LAG:
            raise ValueError("StreamMonitor: lag must be a whole number of hops in 0 .. %d (got %r)" % (MAX_LAG, lag))
        self.lag = int(lag)
        self.alpha = smoothing_factor(time_constant)
        self._alloc(device, lib.nele_mon_state_bytes(self.S))
        call('nele_mon_init', ptr(self.state), c_longlong(self.nbytes), self.S, self.lag, stream())
        self._stats = self._fresh_stats(self.S)

    def _fresh_stats(self, rows):
        s = torch.zeros((rows, NSTATS), dtype=torch.float64, device=self.device)
        s[:, LOUDEST] = -math.inf
        return s

    # ---- streaming
    def process(self, ref, deg=None, add=None, active=None, want=()):
        """ref [streams, nh * 256] float32 (host, pinned host or device): the clean signal, compared ``lag`` hops later; deg: the processed
        signal of this hop, or None: the delayed ref itself; add: what is summed onto deg, the noise at the listener's ear, or None.
        Returns None - the readings stay on the device for read() - unless want names any of 'stats' (float64 [streams, 8], a copy of
        the readings after this call), 'seg' (float64 [streams, nh, 2]: the d of the segments each hop formed, NaN elsewhere and for a
        skipped segment) and 'nseg' (int32 [streams, nh]); the call then returns a tuple in the order asked for.  active: host bool
        sequence [streams] or None (all): inactive slots are neither read nor changed; their rows of seg and nseg are undefined.
        One launch; never blocks the host."""
        want = (want,) if isinstance(want, str) else tuple(want)
        if [n for n in want if n not in WANT] or len(set(want)) != len(want):
            raise ValueError("StreamMonitor.process: want must be distinct names out of %s (got %s)" % (WANT, want))
        shape = tuple(np.shape(ref))
        if len(shape) != 2 or shape[0] != self.S or shape[1] % HOP or shape[1] == 0:
            raise ValueError("StreamMonitor.process: ref must be [%d, nh * 256]" % self.S)
        nh = shape[1] // HOP
        r = self._dev_f32(ref, shape, 'ref')
        d = None if deg is None else self._dev_f32(deg, shape, 'deg')
        n = None if add is None else self._dev_f32(add, shape, 'add')
        act = None if active is None else self._flags(active, "StreamMonitor: active must hold one flag per stream")
        flags = None if act is None else self._dev_bytes(act)
        seg = torch.empty((self.S, nh, 2), dtype=torch.float64, device=self.device) if 'seg' in want else None
        nseg = torch.empty((self.S, nh), dtype=torch.int32, device=self.device) if 'nseg' in want else None
        call('nele_mon_hop', ptr(self.state), c_longlong(self.nbytes), self.S, ptr(r), ptr(d), ptr(n), ptr(flags), nh, self.alpha,
             ptr(self._stats), ptr(seg), ptr(nseg), stream())
        self._count(act, nh)
        if not want:
            return None
        got = {'stats': self._stats.clone() if 'stats' in want else None, 'seg': seg, 'nseg': nseg}
        return tuple(got[name] for name in want)

    def read(self, mapped=False):
        """-> Reading(stats, estoi, last, smoothed, segments, skipped), all on the device and none of them waited for: stats float64
        [streams, 8] (segments counted, sum of d, last d, smoothed d, segments skipped, frames seen, frames kept, the loudest frame in
        dB), estoi = sum / count (NaN before the first counted segment).  mapped: estoi, last and smoothed through the logistic map of
        metrics.mapping_ESTOI_harvard."""
        s = self._stats.clone()
        vals = [s[:, SUM] / s[:, COUNT], s[:, LAST], s[:, SMOOTH]]
        if mapped:
            vals = [map_estoi(v) for v in vals]
        return Reading(s, vals[0], vals[1], vals[2], s[:, COUNT], s[:, SKIPPED])

    def reset(self, slots):
        """Restart the given slots (no history, no loudest frame, readings zero); the other slots are not touched."""
        m = self._slots_mask(slots)
        call('nele_mon_reset', ptr(self.state), c_longlong(self.nbytes), self.S, ptr(self._dev_bytes(m)), stream())
        rows = self._dev_rows(np.nonzero(m)[0])
        self._stats.index_copy_(0, rows, self._fresh_stats(int(m.sum())))
        self.hops[m] = 0


def lag_of(inner):
    """hops by which the output of a RealtimeEnhancer, CompressedEnhancer or LimitedEnhancer is behind its input (streamrate's rule)"""
    if hasattr(inner, 'lag_hops'):
        return int(inner.lag_hops)
    return 2 if hasattr(inner, 'drc') else 1


class MonitoredEnhancer:
    """A ``RealtimeEnhancer``, ``CompressedEnhancer`` or ``LimitedEnhancer`` with a ``StreamMonitor`` beside it: per call
    out = inner.process(clean, noise);  mon.process(clean, out, noise)  - and, with ``baseline``, baseline.process(clean, None, noise),
    the unprocessed signal in the same noise.  The output is the inner object's, bit for bit, and the object stands where the inner one
    does - inside ``EchoCancellingEnhancer`` too, where ``noise`` is the canceller's residual.  ``lag_hops``: the inner object's."""

    def __init__(self, inner, mon, baseline=None):
        self.lag_hops = lag_of(inner)
        for m, what in ((mon, 'the monitor'), (baseline, 'the baseline monitor')):
            if m is None:
                continue
            if m.S != inner.S:
                raise ValueError("MonitoredEnhancer: the enhancer has %d streams, %s %d" % (inner.S, what, m.S))
            if m.lag != self.lag_hops:
                raise ValueError("MonitoredEnhancer: the enhancer's output is %d hops behind its input, %s has lag=%d" % (self.lag_hops, what, m.lag))
        self.inner, self.mon, self.baseline, self.S = inner, mon, baseline, inner.S

    @property
    def device(self):
        return self.mon.device

    def process(self, clean, noise, active=None, debug=None):
        """the inner object's process and its result; the monitors read the same hops"""
        shape = tuple(np.shape(clean))
        if len(shape) == 2 and shape[0] == self.S and shape[1] and shape[1] % HOP == 0:      # (otherwise the inner object says what is wrong)
            clean, noise = self.mon._dev_f32(clean, shape, 'clean'), self.mon._dev_f32(noise, shape, 'noise')
        kw = {} if debug is None else {'debug': debug}
        out = self.inner.process(clean, noise, active=active, **kw)
        self.mon.process(clean, out, noise, active=active)
        if self.baseline is not None:
            self.baseline.process(clean, None, noise, active=active)
        return out

    def finish(self, slots, clean_tail, noise_tail, tail_lengths, debug=None):
        """the inner object's finish; the last, partial hop is not measured"""
        kw = {} if debug is None else {'debug': debug}
        return self.inner.finish(slots, clean_tail, noise_tail, tail_lengths, **kw)

    def reset(self, slots):
        """Restart the given slots in every object."""
        self.inner.reset(slots)
        self.mon.reset(slots)
        if self.baseline is not None:
            self.baseline.reset(slots)

    def benefit(self):
        """smoothed ESTOI of the processed signal minus that of the unprocessed one, float64 [streams] on the device"""
        if self.baseline is None:
            raise ValueError("MonitoredEnhancer.benefit: no baseline monitor was given")
        return self.mon._stats[:, SMOOTH] - self.baseline._stats[:, SMOOTH]


# ------------------------------------------------------------------------------------------------------------------ command line
def monitor_files(clean, noise, inner=None, time_constant=1.0, device='cuda', rows=False):
    """clean, noise: float32 arrays at 16 kHz -> (ESTOI of the processed signal, ESTOI of the unprocessed one) over the whole hops of
    the shorter one, hop by hop through ``inner`` (default: a rule-mode RealtimeEnhancer); rows: also one tuple per hop (time [s],
    last, smoothed and cumulative of the processed signal, then of the unprocessed one)."""
    from .realtime import RealtimeEnhancer
    from .siiopt import SiiOptRule
    nh = min(len(clean), len(noise)) // HOP
    if nh < 1:
        raise ValueError("monitor: the signals hold no whole hop")
    c = torch.from_numpy(np.ascontiguousarray(clean[:nh * HOP], dtype=np.float32)[None])
    n = torch.from_numpy(np.ascontiguousarray(noise[:nh * HOP], dtype=np.float32)[None])
    inner = RealtimeEnhancer(rule=SiiOptRule(), streams=1, device=device) if inner is None else inner
    lag = lag_of(inner)
    chain = MonitoredEnhancer(inner, StreamMonitor(1, lag, time_constant, device), StreamMonitor(1, lag, time_constant, device))
    c, n = chain.mon._dev_f32(c, tuple(c.shape), 'clean'), chain.mon._dev_f32(n, tuple(n.shape), 'noise')
    per_hop = []
    for h in range(nh):
        chain.process(c[:, h * HOP:(h + 1) * HOP], n[:, h * HOP:(h + 1) * HOP])
        if rows:
            per_hop.append(torch.cat([chain.mon._stats[0, :SKIPPED], chain.baseline._stats[0, :SKIPPED]]))
    final = [float(m.read().estoi[0]) for m in (chain.mon, chain.baseline)]
    if not rows:
        return final[0], final[1]
    table = torch.stack(per_hop).cpu().numpy()                                    # the one read-back, after the last hop
    with np.errstate(invalid='ignore'):
        out = [((h + 1) * HOP / 16000.0, t[LAST], t[SMOOTH], t[SUM] / t[COUNT], t[4 + LAST], t[4 + SMOOTH], t[4 + SUM] / t[4 + COUNT])
               for h, t in enumerate(table)]
    return final[0], final[1], out


def build_parser():
    import argparse
    ap = argparse.ArgumentParser(prog='python -m nele_gan_amd.monitor', description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--clean', required=True, help='16 kHz wav: the speech to be played')
    ap.add_argument('--noise', required=True, help='16 kHz wav: the noise at the listener\'s ear')
    ap.add_argument('--chkpt', default=None, help='checkpoint with an enhance-model entry: the generator runs the stream')
    ap.add_argument('--rule', default=None, choices=('siiopt',), help='the SII-optimal rule runs the stream (the default)')
    ap.add_argument('--time-constant', type=float, default=1.0, help='of the smoothed reading, seconds')
    ap.add_argument('--csv', default=None, help='write one row per hop: time, last, smoothed, cumulative - processed, then unprocessed')
    return ap


def main(argv=None):
    from . import dataio
    from .realtime import RealtimeEnhancer
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.chkpt is not None and a.rule is not None:
        ap.error('--chkpt and --rule exclude each other')
    try:
        smoothing_factor(a.time_constant)
    except ValueError:
        ap.error('--time-constant must be a positive number of seconds')
    sig = []
    for path in (a.clean, a.noise):
        wav, sr = dataio.read_wav(path)
        if sr != dataio.fs:
            ap.error('%s is sampled at %d Hz, not %d: convert it first with python -m nele_gan_amd.resample' % (path, sr, dataio.fs))
        sig.append(wav)
    if min(len(s) for s in sig) < HOP:
        ap.error('the files hold no whole hop of %d samples' % HOP)
    inner = None if a.chkpt is None else RealtimeEnhancer(chkpt_path=a.chkpt, streams=1)
    proc, raw, rows = monitor_files(sig[0], sig[1], inner, a.time_constant, rows=True)
    if a.csv:
        with open(a.csv, 'w') as f:
            f.write('time_s,last,smoothed,cumulative,last_unprocessed,smoothed_unprocessed,cumulative_unprocessed\n')
            for row in rows:
                f.write(','.join('%.9g' % v for v in row) + '\n')
    print('%d hops (%s): ESTOI processed %.4f, unprocessed %.4f' % (len(rows), 'generator' if a.chkpt else 'rule siiopt', proc, raw))
    return 0


if __name__ == '__main__':
    import sys
    sys.exit(main())
