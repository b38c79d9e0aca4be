/* libnele_hip.so -- the fourth public header of the same library.  include/nele_hip.h, include/nele_hip_ext.h and include/nele_hip_ext2.h
 * are each fixed at their own set of entry points (tests/test_capi_symbols.py, tests/test_abi_ext_cpu.py and tests/test_abi_ext2_cpu.py
 * count them).  Entry points added after those go here; the conventions are those of nele_hip.h (device pointers unless named _host,
 * caller-owned memory, `stream` a hipStream_t passed as void*, status 0 / -1 .. -5 with nele_last_error_string()).  tools/gen_abi.py
 * generates nele_gan_amd/_abi_ext3.py from this file as it generates the other three; nele_gan_amd/_lib.py binds all four.  None of
 * these is a job-table operation.
 * So far: the stream converter on a hop schedule (nele_sched_stream_*), for 44.1 kHz and its family.
 */
#ifndef NELE_HIP_EXT3_H
#define NELE_HIP_EXT3_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- stream-rate conversion on a hop schedule (csrc/resample_sched.hip) -------------------------------------------
 * nele_resample_stream_* of nele_hip.h serves the device rates at which a 256-sample hop at 16 kHz is a whole number of device samples.
 * These serve every rate section 12 admits: the 16 kHz side moves 256 samples per hop, the device side
 *   n(g) = floor((g + 1) r) - floor(g r)   samples in the hop at schedule position g,   r = 256 sr_dev / 16000 = num / P in lowest terms
 * (705, 706, 705, 706, 706 at 44.1 kHz; P = 1 at the whole-hop rates).  up / down = sr_out / sr_in in lowest terms as in
 * nele_resample_var; to16k != 0: the output side is the 16 kHz side.  The table hp_dev [up][K] float64 is nele_resample_taps' layout 1,
 * read from global memory (from LDS where it is at most 16 KiB).
 * A slot keeps H input samples of history (float32) and its lead L: relative to the first input sample of its next hop, output j of
 * that hop is the offline formula at c = L + j down.  Output m of a slot's stream is y[m - D] of nele_resample_var for everything fed
 * to the slot since its reset, bit for bit.  A slot's bits do not depend on max_streams, on the grouping of hops into calls, on pos as
 * such or on the other slots.
 * nele_sched_stream_plan: info_host [NELE_SCHED_INFO] int, NELE_SCHED_I_*.  No GPU call.  -1 where the delay D is longer than the
 *   shortest output hop.
 * nele_sched_stream_widths: the samples per row of a call of nh hops from schedule position pos (0 .. P - 1): 256 nh on the 16 kHz
 *   side, floor((pos + nh) r) - floor(pos r) on the other.  No GPU call.
 * `state` (nele_sched_stream_state_bytes(max_streams, H) bytes, 256-byte aligned): a 256-byte header (max_streams, K, up, down, to16k,
 *   H, L0), then one record of nele_sched_stream_record_bytes(H) bytes per slot: int lead, three reserved ints, float [H].
 *   nele_sched_stream_init lays it out and resets every slot (zero history, lead = L0); nele_sched_stream_reset resets the slots with
 *   slots[b] != 0 (NULL = all).  The same (max_streams, up, down, K, to16k) in every call on one state: a kernel given others touches
 *   nothing.
 * nele_sched_stream_hop: x [max_streams] rows of x_stride float32, y [max_streams] rows of y_stride; nh hops from position pos, the
 *   widths nele_sched_stream_widths gives.  active [max_streams] (bytes, NULL = all): inactive slots are neither read nor written and
 *   their columns of y are left as they were.  The positions are the caller's bookkeeping: every active slot must stand at pos.  A slot
 *   whose lead does not fit the call (L < -E up, or L + (n_out - 1) down >= n_in up: it would read outside history + row) gets NaN
 *   in its columns of y and keeps its record.
 * Bad host arguments are -1 before any GPU call; the *_bytes functions return -1 on bad arguments and make no HIP call.  Nothing is
 * allocated; there is no workspace. */
#define NELE_SCHED_INFO 9              /* ints nele_sched_stream_plan fills */
#define NELE_SCHED_I_K 0               /* table width */
#define NELE_SCHED_I_D 1               /* delay, output samples */
#define NELE_SCHED_I_L0 2              /* lead behind a reset */
#define NELE_SCHED_I_E 3               /* history samples beyond K - 1 */
#define NELE_SCHED_I_H 4               /* history length K - 1 + E */
#define NELE_SCHED_I_RNUM 5            /* r = RNUM / P */
#define NELE_SCHED_I_P 6               /* the schedule's period */
#define NELE_SCHED_I_HOP_MIN 7         /* shortest hop on the side that is not 16 kHz */
#define NELE_SCHED_I_HOP_MAX 8         /* longest */
int nele_sched_stream_plan(int up, int down, int zeros, int to16k, int* info_host);
int nele_sched_stream_widths(int up, int down, int to16k, int pos, int nh, long long* n_in, long long* n_out);
long long nele_sched_stream_record_bytes(int H);
long long nele_sched_stream_state_bytes(int max_streams, int H);
int nele_sched_stream_init(void* state, long long state_bytes, int max_streams, int up, int down, int K, int to16k, void* stream);
int nele_sched_stream_reset(void* state, long long state_bytes, int max_streams, int up, int down, int K, int to16k,
                            const unsigned char* slots, void* stream);
int nele_sched_stream_hop(void* state, long long state_bytes, int max_streams, int up, int down, int K, int to16k, const double* hp_dev,
                          const float* x, long long x_stride, const unsigned char* active, int nh, int pos, float* y, long long y_stride,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif
