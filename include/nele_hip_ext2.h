/* libnele_hip.so -- the third public header of the same library.  include/nele_hip.h is fixed at its own set of entry points (the
 * job-table operation ids of csrc/plan_ops.inc derive from it) and include/nele_hip_ext.h at the 19 of its three features (the bulk-delay
 * search, its tracking mode, the residual-echo suppressor: tests/test_abi_ext_cpu.py counts them).  Entry points added after those go
 * here; the conventions are those of nele_hip.h (device pointers unless named _host, caller-owned memory, `stream` a hipStream_t passed
 * as void*, status 0 / -1 .. -5 with nele_last_error_string(), fixed-order reductions).  tools/gen_abi.py generates
 * nele_gan_amd/_abi_ext2.py from this file as it generates _abi.py and _abi_ext.py from the other two; nele_gan_amd/_lib.py binds all
 * three.  None of these is a job-table operation.
 * The real-time echo path's clock-drift compensator (nele_drift_*): eight entry points, which tests/test_abi_ext2_cpu.py counts.  Later
 * entry points go into include/nele_hip_ext3.h.
 */
#ifndef NELE_HIP_EXT2_H
#define NELE_HIP_EXT2_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- clock drift between playback and capture, followed ahead of the echo canceller (csrc/drift.hip) ----------------------------------
 * Per stream slot: a fractional, moving delay line that stands where the bulk search's whole-hop delay line stands.  It takes the
 * whole-hop delay the search found (base_hops, on the device), hands `played` on delayed by tau(t) samples through a 64-phase, 64-tap
 * Kaiser-windowed sinc table with linear blending between neighbouring phases, and moves tau and its rate with a second-order loop on
 * the phase slope between a fast and a slow average of the SCOT-weighted cross-spectrum of the microphone against its own output
 * (DESIGN.md section 19 is the arithmetic; 256-sample hops, float64 on float32 inputs).  rate is in samples of delay per sample: the
 * capture clock runs fast by -1e6 rate ppm.
 * `blocks` = Q, 2 .. NELE_BULK_MAX_BLOCKS of nele_hip_ext.h: the search's own value; the slot keeps a ring of Q + 4 hops of `played`.
 * `state` (nele_drift_state_bytes(max_streams, blocks) bytes, 256-byte aligned) holds a header, the table (65 x 64 float64, computed
 * on the device by nele_drift_init) and one record of nele_drift_stream_record_bytes(blocks) bytes per slot; nele_drift_init lays it out
 * and clears every slot, nele_drift_reset clears the slots with slots[b] != 0 (NULL = all).  The same (max_streams, blocks) in every
 * call on one state: a kernel given another pair touches nothing.
 * nele_drift_hop: mic / played / aligned [max_streams][nh * 256] float32, hop h of the call in columns [256 h, 256 h + 256).
 *   base_hops [max_streams] int32: read once per call by each active slot; a value b in 0 .. blocks - 1 that differs from the one the
 *   slot last took SNAPS it (tau = max(256 b, 31), the estimator cleared, rate and the ring kept); any other value (-1 = still
 *   searching) changes nothing.  aligned: exact zeros until the slot's first snap.  snapped [max_streams] (bytes, or NULL) is written
 *   by every call: 1 for an active slot that snapped in this call, 0 for every other slot.  active [max_streams] (bytes, NULL = all):
 *   inactive slots are neither read nor written and their columns of aligned are left as they were.  adapt [max_streams] (bytes,
 *   NULL = all): a slot that does not adapt warps with the tau and rate it has and still runs the estimator.
 *   0 < lam_fast < lam_slow < 1, kp >= 0, ki >= 0, finite (0.9, 0.99, 0.02 and 5e-4 are the values the loop was tried with).  A
 *   slot's outputs and state are the same bits whatever nh per call, max_streams and the other slots are, given the same base_hops
 *   on every call.
 * nele_drift_set_rate: rate_dev [max_streams] float64: the slots with slots[b] != 0 (NULL = all) take rate_dev[b]; a value outside
 *   +-NELE_DRIFT_MAX_RATE (or not a number) cannot be reported - the values are not read back - and leaves its slot unchanged.
 * nele_drift_status: info [max_streams][NELE_DRIFT_INFO] float64: per slot NELE_DRIFT_I_*.
 * nele_drift_taps: taps_out_dev [65][64] float64: the table as the state holds it.
 * Bad host arguments are -1 before any GPU call; the *_bytes functions return -1 on bad arguments and make no HIP call.  Nothing is
 * allocated; there is no workspace. */
#define NELE_DRIFT_PHASES 64           /* fractional-delay phases: the table has NELE_DRIFT_PHASES + 1 rows */
#define NELE_DRIFT_TAPS 64             /* taps per phase */
#define NELE_DRIFT_BETA 8.0            /* the Kaiser window's beta */
#define NELE_DRIFT_SMOOTH 0.9          /* S <- NELE_DRIFT_SMOOTH S + (1 - NELE_DRIFT_SMOOTH) |.|^2 for the powers S_d, S_u */
#define NELE_DRIFT_EPS 1e-6            /* c = D conj(U) / sqrt(S_d S_u + NELE_DRIFT_EPS): the units of NELE_BULK_EPS */
#define NELE_DRIFT_TINY 1e-12          /* the guard in the phase-slope ratio */
#define NELE_DRIFT_WARM 32             /* hops of the estimator before the loop closes */
#define NELE_DRIFT_MAX_RATE 1e-3       /* |rate| <= 1000 ppm */
#define NELE_DRIFT_INFO 6              /* float64 values per slot in nele_drift_status's info */
#define NELE_DRIFT_I_TAU 0             /* samples */
#define NELE_DRIFT_I_RATE 1            /* samples of delay per sample */
#define NELE_DRIFT_I_DELTA 2           /* the last hop's phase-slope estimate, samples */
#define NELE_DRIFT_I_N 3               /* hops the estimator has seen since the last snap */
#define NELE_DRIFT_I_BASE 4            /* the whole-hop delay the slot last took, -1 = none yet */
#define NELE_DRIFT_I_SNAPS 5           /* snaps since the reset */
long long nele_drift_state_bytes(int max_streams, int blocks);
long long nele_drift_stream_record_bytes(int blocks);
int nele_drift_init(void* state, long long state_bytes, int max_streams, int blocks, void* stream);
int nele_drift_reset(void* state, long long state_bytes, int max_streams, int blocks, const unsigned char* slots, void* stream);
int nele_drift_set_rate(void* state, long long state_bytes, int max_streams, int blocks, const unsigned char* slots, const double* rate_dev,
                        void* stream);
int nele_drift_hop(void* state, long long state_bytes, int max_streams, int blocks, const float* mic, const float* played,
                   const int* base_hops, const unsigned char* active, const unsigned char* adapt, int nh, double lam_fast, double lam_slow,
                   double kp, double ki, float* aligned, unsigned char* snapped, void* stream);
int nele_drift_status(const void* state, long long state_bytes, int max_streams, int blocks, double* info, void* stream);
int nele_drift_taps(const void* state, long long state_bytes, int max_streams, int blocks, double* taps_out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
