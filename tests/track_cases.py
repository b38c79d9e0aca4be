"""The delay-tracking scenarios shared by tests/test_track_cpu.py and tests/test_track_gpu.py: tests/bulk_cases.py's audio tiled to any
number of hops, the echo switched at a given hop from one path (``bulk_a`` samples of pure delay) to another, redrawn, path (``bulk_b``),
an optional stretch without echo, the microphone = echo + noise at a stated echo-to-noise ratio; and the echo-free microphones of
bulk_cases.negatives() tiled in the same way."""
import numpy as np

import aec_cases as C
import bulk_cases as BC

HOP = C.HOP
# tests/test_track_gpu.py's parity scenarios (tests/test_track_cpu.py checks what the reference does on them): Q -> per slot (bulk before,
# bulk after, ENR dB, path seed, taps, T60, jump hop or None); slot i's far end is shifted by 4001 i.  Short searches for short tests:
GPU_RATIO, GPU_HOLD, GPU_PATIENCE, GPU_JUMP, GPU_HOPS = 8.0, 8, 48, 110, 300
GPU_SCENARIOS = {
    3: [(600, 100, 10.0, 33, 150, 0.03, GPU_JUMP), (700, 40, 10.0, 34, 150, 0.03, GPU_JUMP), (400, 400, 10.0, 32, 200, 0.03, None)],
    8: [(1900, 300, 10.0, 85, 700, 0.08, GPU_JUMP), (40, 1500, 10.0, 81, 700, 0.08, GPU_JUMP), (1000, 1000, 10.0, 83, 700, 0.08, None),
        (700, 1900, 10.0, 82, 300, 0.04, GPU_JUMP), (1500, 40, 0.0, 84, 300, 0.04, GPU_JUMP)],
    32: [(5000, 1000, 0.0, 6, 700, 0.08, GPU_JUMP), (2000, 7000, 10.0, 5, 700, 0.08, GPU_JUMP)],
}


def tiled(x, n, shift=0):
    x = np.roll(x, shift)
    return np.tile(x, -(-n // len(x)))[:n]


def scenario(bulk_a, bulk_b, enr_db, seed, jump_hop, hops, taps=700, t60=0.08, shift=0, mute=None):
    """-> dict: played (float32), echo, noise (float64), mic = float32(echo + noise), h_a, h_b, jump_hop.  Up to hop ``jump_hop`` the echo
    is `played` through bulk_cases.path(seed, taps, t60, bulk_a), from it on through path(seed + 1000, taps, t60, bulk_b) (jump_hop None:
    one path throughout); mute = (first hop, end hop): no echo there.  The noise is scaled against the echo of the first path over the
    whole length (both paths have sum h^2 = 0.25)."""
    far, near = C.far_and_near()
    n = hops * HOP
    played = tiled(far, n, shift).astype(np.float32)
    h_a = BC.path(seed, taps, t60, bulk_a)
    echo_a = np.convolve(played.astype(np.float64), h_a)[:n]
    echo, h_b = echo_a.copy(), None
    if jump_hop is not None:
        h_b = BC.path(seed + 1000, taps, t60, bulk_b)
        echo[jump_hop * HOP:] = np.convolve(played.astype(np.float64), h_b)[jump_hop * HOP:n]
    noise = C.scale_to_enr(echo_a, tiled(near, n, 2 * shift), enr_db)
    if mute is not None:
        echo[mute[0] * HOP:mute[1] * HOP] = 0.0
    return {'played': played, 'h_a': h_a, 'h_b': h_b, 'echo': echo, 'noise': noise, 'mic': (echo + noise).astype(np.float32), 'jump_hop': jump_hop}


def negatives(hops):
    """-> [(name, mic, played)] float32, ``hops`` hops each: the 24 echo-free microphones of bulk_cases.negatives() (white noise, the toy
    noise shifted, the reversed far end shifted) against the far end, tiled"""
    n = hops * HOP
    return [(name, tiled(mic, n).astype(np.float32), tiled(played, n).astype(np.float32)) for name, mic, played in BC.negatives()[:24]]


def main_tap_after_alignment(bulk, delay_hops):
    """where the path's main tap lies once `played` comes ``delay_hops`` hops late"""
    return bulk - delay_hops * HOP
