/* libnele_hip.so -- the ninth public header of the same library.  include/nele_hip.h, include/nele_hip_ext.h, include/nele_hip_ext2.h,
 * include/nele_hip_ext3.h, include/nele_hip_ext4.h, include/nele_hip_ext5.h, include/nele_hip_ext6.h and include/nele_hip_ext7.h are each
 * fixed at their own set of entry points (tests/test_capi_symbols.py, tests/test_abi_ext_cpu.py .. tests/test_abi_ext7_cpu.py count
 * them).  Entry points added after those go here; the conventions are those of nele_hip.h (device pointers unless named _host,
 * caller-owned memory, `stream` a hipStream_t passed as void*, status 0 / -1 .. -5 with nele_last_error_string()).  tools/gen_abi.py
 * generates nele_gan_amd/_abi_ext8.py from this file as it generates the other eight; nele_gan_amd/_lib.py binds all nine.  None of
 * these is a job-table operation.
 * So far: the up-converter on a hop schedule that carries the band above 8 kHz past the enhancer (nele_hbsched_*), for 44.1 kHz and its
 * family.
 */
#ifndef NELE_HIP_EXT8_H
#define NELE_HIP_EXT8_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- 16 kHz -> device rate on a hop schedule with the high band carried (csrc/highband_sched.hip) ----------------
 * nele_hbup_* of nele_hip_ext7.h serves the device rates at which a 256-sample hop at 16 kHz is a whole number of device samples and
 * the path's delay a whole number too.  These serve every rate above 16 kHz that nele_sched_stream_* of nele_hip_ext3.h converts.
 * The path's delay, (D_down + lam) up / down + D_up device samples (D_down the down-converter's delay at 16 kHz, lam = 256 lag_hops
 * the enhancer's, D_up the up-converter's), is not a whole number there: 4414/5 at 44.1 kHz.  The up-converter is therefore run
 * s / down of a device sample late, s = (-(D_down + lam) up) mod down: its slots start at the lead L0 - s where nele_sched_stream_*'s
 * start at L0, every output the same polyphase sum taken s ticks of 1 / down later.  Then Lx = ((D_down + lam) up + s) / down + D_up
 * is a whole number and, per stream, with zeros before its start:
 *   d[n] = fmaf(-g, low[n - lam], enh[n])                      float32, at 16 kHz
 *   u[m] = the scheduled up-conversion of d from the lead L0 - s   (nele_sched_stream_hop's sum: float64, k ascending, one fma per term)
 *   y[m] = fmaf(g, x[m - Lx], (float)u[m])                     float32, at the device rate
 * nele_hbsched_plan: info_host [NELE_HBSCHED_INFO] int, NELE_HBSCHED_I_*, for the up-converter up / down with `zeros`, lag_hops hops of
 *   256 samples between low and enh, and the down-converter's delay d_down (NELE_SCHED_I_D of the opposite direction).  No GPU call.
 * `state` (nele_hbsched_state_bytes(max_streams, H, lam, Lx) bytes, 256-byte aligned): a 256-byte header (max_streams, K, up, down, H,
 *   L0 - s, lam, Lx), then one record of nele_hbsched_record_bytes(H, lam, Lx) bytes per slot: int lead, three reserved ints, then
 *   float32: the last H of d, the last lam of low, the last Lx of x.  nele_hbsched_init lays it out and resets every slot (zeros, lead
 *   = L0 - s); nele_hbsched_reset resets the slots with slots[b] != 0 (NULL = all).  The same (max_streams, up, down, K, s, lam, Lx) in
 *   every call on one state: a kernel given others touches nothing.
 * nele_hbsched_hop: nh hops from schedule position pos (0 .. P - 1).  enh, low [max_streams] rows of 256 nh float32, enh_stride /
 *   low_stride apart; x, y [max_streams] rows of floor((pos + nh) r) - floor(pos r) float32 (nele_sched_stream_widths), x_stride /
 *   y_stride apart; y overlaps none of the inputs.  gain [max_streams] float32, g of each slot, or NULL (1 for all).  active
 *   [max_streams] bytes or NULL (all): a slot with active[b] == 0 is neither read nor written.  The positions are the caller's
 *   bookkeeping: every active slot must stand at pos.  A slot whose lead does not fit the call (L < -E up, or L + (n_out - 1) down >=
 *   256 nh up: it would read outside history + row) gets NaN in its columns of y and keeps its record.
 * One launch per call.  A slot's outputs and state are the same bits whatever the grouping of hops into calls, max_streams and the
 * other slots are.  Bad host arguments are -1 with the function's name before any GPU call; the *_bytes functions make no HIP call (-1
 * for a bad argument).  The limits on lam and Lx are NELE_HBUP_MAX_LAG16 and NELE_HBUP_MAX_LAG of nele_hip_ext7.h.  Nothing is
 * allocated. */
#define NELE_HBSCHED_INFO 12           /* ints nele_hbsched_plan fills */
#define NELE_HBSCHED_I_K 0             /* table width */
#define NELE_HBSCHED_I_D_UP 1          /* the up-converter's delay, device samples */
#define NELE_HBSCHED_I_S 2             /* the shift s, ticks of 1 / down of a device sample */
#define NELE_HBSCHED_I_L0 3            /* lead behind a reset: L0 - s */
#define NELE_HBSCHED_I_E 4             /* history samples of d beyond K - 1 */
#define NELE_HBSCHED_I_H 5             /* history length K - 1 + E */
#define NELE_HBSCHED_I_LAM 6           /* 256 lag_hops */
#define NELE_HBSCHED_I_LX 7            /* how far y is behind x, device samples */
#define NELE_HBSCHED_I_RNUM 8          /* r = RNUM / P device samples per hop */
#define NELE_HBSCHED_I_P 9             /* the schedule's period */
#define NELE_HBSCHED_I_HOP_MIN 10      /* shortest hop at the device rate */
#define NELE_HBSCHED_I_HOP_MAX 11      /* longest */
int nele_hbsched_plan(int up, int down, int zeros, int lag_hops, int d_down, int* info_host);
long long nele_hbsched_record_bytes(int H, int lam, int Lx);
long long nele_hbsched_state_bytes(int max_streams, int H, int lam, int Lx);
int nele_hbsched_init(void* state, long long state_bytes, int max_streams, int up, int down, int K, int s, int lam, int Lx, void* stream);
int nele_hbsched_reset(void* state, long long state_bytes, int max_streams, int up, int down, int K, int s, int lam, int Lx,
                       const unsigned char* slots, void* stream);
int nele_hbsched_hop(void* state, long long state_bytes, int max_streams, int up, int down, int K, int s, int lam, int Lx, const double* hp_dev,
                     const float* enh, long long enh_stride, const float* low, long long low_stride, const float* x, long long x_stride,
                     const float* gain, const unsigned char* active, int nh, int pos, float* y, long long y_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif
