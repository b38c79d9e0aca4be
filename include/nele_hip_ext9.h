/* libnele_hip.so -- the tenth public header of the same library.  include/nele_hip.h, include/nele_hip_ext.h, include/nele_hip_ext2.h,
 * include/nele_hip_ext3.h, include/nele_hip_ext4.h, include/nele_hip_ext5.h, include/nele_hip_ext6.h, include/nele_hip_ext7.h and
 * include/nele_hip_ext8.h are each fixed at their own set of entry points (tests/test_capi_symbols.py, tests/test_abi_ext_cpu.py ..
 * tests/test_abi_ext8_cpu.py count them).  Entry points added after those go here; the conventions are those of nele_hip.h (device
 * pointers unless named _host, caller-owned memory, `stream` a hipStream_t passed as void*, status 0 / -1 .. -5 with
 * nele_last_error_string()).  tools/gen_abi.py generates nele_gan_amd/_abi_ext9.py from this file as it generates the other nine;
 * nele_gan_amd/_lib.py binds all ten.  None of these is a job-table operation.
 * So far: the look-ahead true-peak limiter, the last stage of the real-time path (nele_lim_*).
 */
#ifndef NELE_HIP_EXT9_H
#define NELE_HIP_EXT9_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- look-ahead true-peak limiter, many concurrent streams (csrc/limiter.hip) -----------------------------------
 * NELE_LIM_HOP samples per hop at 16 kHz, float64 between the float32 input and the float32 output.  With s = drive * x (zeros before
 * the stream's start) and, per sample, p the largest of |s| and of the six values the taps interpolate at the quarter points on either
 * side of it (or |s| alone without taps):  r = p > ceiling ? ceiling / p : 1;  m[n] = min r[n .. n + lookahead];
 * d[n] = max(1 - m[n], rel d[n - 1]), q = 1 - d;  g[n] = min((q[n - lookahead] + .. + q[n]) / (lookahead + 1), r[n]);  out = (float)(g s), held to
 * +-cf, the largest float32 <= ceiling, by a clamp that finite input never reaches.  The recursion starts `lookahead` samples before the
 * stream does.  THE OUTPUT IS ONE HOP LATE: a slot's first hop yields NELE_LIM_HOP zeros, hop h >= 1 yields hop h - 1.
 *   state    one caller-owned allocation of nele_lim_state_bytes(max_streams, lookahead) bytes, 256-byte aligned: a 256-byte header
 *            (max_streams, the record's bytes, lookahead, 262), then one record of nele_lim_stream_record_bytes(lookahead) per slot:
 *            a counter that stops at 2 at byte 0, d at byte 64, the last 262 input samples (float32) at byte 128 and the last
 *            `lookahead` values of q (float64) at byte 1184, rounded up to a multiple of 256 bytes.  All zero after init or reset.
 *            The same lookahead in every call on one state: a kernel given another touches nothing.
 *   x, out   [max_streams][nh * NELE_LIM_HOP] float32; active [max_streams] bytes or null (all): a slot with active[b] == 0 is neither
 *            read nor written - its state, its columns of out, gain and peak stay as they are.
 *   ceiling  > 0, finite; drive > 0, finite; lookahead 1 .. NELE_LIM_MAX_LOOKAHEAD samples; rel, the release factor per sample, in [0, 1).
 *   taps_host  host, [NELE_LIM_TAPS] float64: f_k[m] at [12 (k - 1) + m + 5], k = 1 .. 3, m = -5 .. 6; or null: sample peaks only.
 *   gain     [max_streams][nh * NELE_LIM_HOP] float64 or null: g on every output sample (0 in a slot's first hop).
 *   peak     [max_streams][nh] float64 or null: the emitted hop's largest p (0 in a slot's first hop).
 * One launch per call.  A slot's outputs and state are the same bits whatever nh per call, max_streams and the other slots are.
 * Bad host arguments are -1 with the function's name before any GPU call; the *_bytes functions make no HIP call (-1 for a bad
 * argument).  Nothing is allocated. */
#define NELE_LIM_HOP 256               /* samples per hop */
#define NELE_LIM_MAX_LOOKAHEAD 192     /* samples: the emitted hop reads lookahead + 6 samples of the newest one */
#define NELE_LIM_TAPS 36               /* doubles in taps_host: three quarter-sample interpolators of twelve taps */
long long nele_lim_state_bytes(int max_streams, int lookahead);
long long nele_lim_stream_record_bytes(int lookahead);
int nele_lim_init(void* state, long long state_bytes, int max_streams, int lookahead, void* stream);
int nele_lim_reset(void* state, long long state_bytes, int max_streams, int lookahead, const unsigned char* slots, void* stream);
int nele_lim_hop(void* state, long long state_bytes, int max_streams, const float* x, const unsigned char* active, int nh, double ceiling,
                 double drive, int lookahead, double rel, const double* taps_host, float* out, double* gain, double* peak, void* stream);

#ifdef __cplusplus
}
#endif
#endif
