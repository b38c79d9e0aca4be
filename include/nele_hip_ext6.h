/* libnele_hip.so -- the seventh public header of the same library.  include/nele_hip.h, include/nele_hip_ext.h, include/nele_hip_ext2.h,
 * include/nele_hip_ext3.h, include/nele_hip_ext4.h and include/nele_hip_ext5.h are each fixed at their own set of entry points
 * (tests/test_capi_symbols.py, tests/test_abi_ext_cpu.py .. tests/test_abi_ext5_cpu.py count them).  Entry points added after those go
 * here; the conventions are those of nele_hip.h (device pointers unless named _host, caller-owned memory, `stream` a hipStream_t passed
 * as void*, status 0 / -1 .. -5 with nele_last_error_string()).  tools/gen_abi.py generates nele_gan_amd/_abi_ext6.py from this file as
 * it generates the other six; nele_gan_amd/_lib.py binds all seven.  None of these is a job-table operation.
 * So far: the per-stream dynamic range compressor of the real-time path (nele_drc_*).
 */
#ifndef NELE_HIP_EXT6_H
#define NELE_HIP_EXT6_H
#include "nele_hip.h" /* nele_ssdrc_params */
#ifdef __cplusplus
extern "C" {
#endif

/* ---- causal dynamic range compression, many concurrent streams (csrc/drc.hip) -----------------------------------
 * Stage 2 of SSDRC (nele_ssdrc_compress) on a live stream, NELE_DRC_HOP samples per hop, float64 between the
 * float32 input and the float32 output: the Hilbert envelope and its 161-sample centred mean with 144 samples of look-ahead, the
 * attack / release recursion carried across hops, the static curve through the knots - against a reference level that is e0_ratio
 * times a decaying maximum of the envelope (factor rho per hop) where the offline stage takes the utterance's maximum, or a fixed
 * level per stream - and an equaliser that brings the output's recursive energy (factor lam per hop) to the input's, its gain moved
 * linearly over the hop.  THE OUTPUT IS ONE HOP LATE: a slot's first hop yields NELE_DRC_HOP zeros, hop h >= 1 yields hop h - 1.
 *   state    one caller-owned allocation of nele_drc_state_bytes(max_streams) bytes, 256-byte aligned: a header, then one record of
 *            nele_drc_stream_record_bytes() per slot (the last 400 input samples, five doubles and a counter that stops at 2).
 *   x, out   [max_streams][nh * NELE_DRC_HOP] float32; active [max_streams] bytes or null (all): a slot with active[b] == 0 is neither
 *            read nor written - its state, its columns of out, gain and level stay as they are.
 *   params   host: attack, release, e0_ratio and the knots are used; the other fields are not read.
 *   rho, lam the per-hop factors exp(-0.016 / tau), in [0, 1); equalise != 0 switches the equaliser on.
 *   ref_level [max_streams] float64 or null: the fixed reference level e0 of each slot (a value that is not > 0 passes the slot's
 *            signal through); null: e0 = e0_ratio * M.
 *   gain     [max_streams][nh * NELE_DRC_HOP] float64 or null: the total gain on every output sample (0 in a slot's first hop).
 *   level    [max_streams][nh] float64 or null: e0 of every hop (0 in a slot's first hop).
 * One launch per call.  A slot's outputs and state are the same bits whatever nh per call, max_streams and the other slots are.
 * Bad host arguments are -1 with the function's name before any GPU call; the *_bytes functions make no HIP call (-1 for a bad
 * max_streams).  Nothing is allocated. */
#define NELE_DRC_HOP 256               /* samples per hop */
#define NELE_DRC_HIST 400              /* input samples a record keeps: 256 + 80 + 64 */
#define NELE_DRC_LOOKAHEAD 144         /* samples of the newest hop the emitted hop reads: 80 + 64 */
long long nele_drc_state_bytes(int max_streams);
long long nele_drc_stream_record_bytes(void);
int nele_drc_init(void* state, long long state_bytes, int max_streams, void* stream);
int nele_drc_reset(void* state, long long state_bytes, int max_streams, const unsigned char* slots, void* stream);
int nele_drc_hop(void* state, long long state_bytes, int max_streams, const float* x, const unsigned char* active, int nh,
                 const nele_ssdrc_params* params, double rho, double lam, int equalise, const double* ref_level, float* out, double* gain,
                 double* level, void* stream);

#ifdef __cplusplus
}
#endif
#endif
