/* libnele_hip.so -- the second public header of the same library: entry points added after the 198 of include/nele_hip.h, whose set is
 * fixed (its tests count them and the job-table operation ids of csrc/plan_ops.inc derive from it).  New entry points go here; the
 * conventions are those of nele_hip.h (device pointers unless named _host, caller-owned memory, `stream` a hipStream_t passed as void*,
 * status 0 / -1 .. -5 with nele_last_error_string(), fixed-order reductions).  tools/gen_abi.py generates nele_gan_amd/_abi_ext.py from
 * this file as it generates _abi.py from nele_hip.h; nele_gan_amd/_lib.py binds both.  None of these is a job-table operation.
 * So far: the real-time echo path's bulk-delay search (nele_bulk_*), its tracking mode (nele_track_*) and the residual-echo suppressor
 * (nele_res_*).
 */
#ifndef NELE_HIP_EXT_H
#define NELE_HIP_EXT_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- bulk-delay search and alignment ahead of the echo canceller (csrc/bulkdelay.hip) ------------------------------------------------
 * Per stream slot: find the whole number of 256-sample hops by which the loudspeaker's signal reaches the microphone late, and hand
 * `played` on delayed by it, so that nele_aec_hop's partitions cover the room's tail and not the device's buffers (DESIGN.md section 16
 * is the arithmetic).  `blocks` = Q, 2 .. NELE_BULK_MAX_BLOCKS, one value per state: the search covers main-tap delays up to
 * 256 Q - 1 samples.  While a slot searches, each hop adds the SCOT-weighted cross-spectrum of the microphone's block against each of
 * the last Q far-end blocks to a sum decayed by `lambda`; the energy e_q of the constrained inverse transform of sum q is that of the
 * cross-correlation at lags 256 q .. 256 q + 255.  The slot locks once one block q* has held e_q* (Q - 1) >= ratio * (sum of the
 * others) for `hold` hops in a row, at delay max(q* - 1, 0) hops; from that hop on it does no search work.
 * `state` (nele_bulk_state_bytes(max_streams, blocks) bytes, 256-byte aligned) holds a header and one record of
 * nele_bulk_stream_record_bytes(blocks) bytes per slot; nele_bulk_init lays it out and clears every slot, nele_bulk_reset clears the
 * slots with slots[b] != 0 (NULL = all), which starts their search afresh.  The same (max_streams, blocks) in every call on one state:
 * a kernel given another pair touches nothing.
 * nele_bulk_hop: mic / played / aligned [max_streams][nh * 256] float32, hop h of the call in columns [256 h, 256 h + 256).  aligned:
 *   exact zeros while the slot searches, then `played` of `delay` hops ago, bit for bit (the hop on which the lock falls included).
 *   delay_hops [max_streams] (or NULL): each active slot's delay after the call, -1 = still searching.  active [max_streams] (bytes,
 *   NULL = all): inactive slots are neither read nor written and their output columns and delay_hops entries are left as they were.
 *   0 < lambda < 1, ratio > 1, hold >= 1 (0.99, 8.0 and 16 are the values the search was tried with).  A slot's outputs and state are
 *   the same bits whatever nh per call, max_streams and the other slots are.
 * nele_bulk_set_delay: locks the slots with slots[b] != 0 (NULL = all) at delay_hops[b] hops, a delay the integrator knows; no search
 *   runs and the delay line is kept.  delay_hops[b] must be in 0 .. blocks - 1: the values are on the device and are not read back, so
 *   an out-of-range value cannot be reported - it leaves its slot unchanged.
 * nele_bulk_status (monitoring and tests; every output may be NULL): per slot the delay (-1 = searching), the hops seen while
 *   searching, the block energies of the last evaluated hop, energies [max_streams][blocks], and its conf = e_q* (Q - 1) / rest.
 * Bad host arguments are -1 before any GPU call; the *_bytes functions return -1 on bad arguments and make no HIP call.  Nothing is
 * allocated; there is no workspace. */
#define NELE_BULK_MAX_BLOCKS 64
#define NELE_BULK_SMOOTH 0.9           /* S <- NELE_BULK_SMOOTH S + (1 - NELE_BULK_SMOOTH) |.|^2 for the powers S_d, S_x of the weighting */
#define NELE_BULK_EPS 1e-6             /* D' = D / sqrt(S_d S_x + NELE_BULK_EPS): absolute, in units of (unnormalised 512-point power)^2 of
                                          full-scale (+-1) signals */
long long nele_bulk_state_bytes(int max_streams, int blocks);
long long nele_bulk_stream_record_bytes(int blocks);
int nele_bulk_init(void* state, long long state_bytes, int max_streams, int blocks, void* stream);
int nele_bulk_reset(void* state, long long state_bytes, int max_streams, int blocks, const unsigned char* slots, void* stream);
int nele_bulk_set_delay(void* state, long long state_bytes, int max_streams, int blocks, const unsigned char* slots, const int* delay_hops,
                        void* stream);
int nele_bulk_hop(void* state, long long state_bytes, int max_streams, int blocks, const float* mic, const float* played,
                  const unsigned char* active, int nh, double lambda, double ratio, int hold, float* aligned, int* delay_hops, void* stream);
int nele_bulk_status(const void* state, long long state_bytes, int max_streams, int blocks, int* delay_hops, int* hops_searched,
                     double* energies, double* conf, void* stream);

/* ---- a bulk-delay search that follows the delay when it moves after the lock (csrc/bulkdelay.hip) -------------------------------------
 * Per stream slot: the delay line and the search of nele_bulk_* (the same kernel in its tracking mode and the
 * same record layout), with the search started again from a cleared state behind every lock, over and over (DESIGN.md section 18 is
 * the arithmetic).  A background search that reaches `hold` hops in a row at block q*: the first one locks the slot at
 * max(q* - 1, 0) hops; later ones confirm the delay when
 * 0 <= q* - delay <= 2 (the main tap still lies in the 768 samples section 16 promises) and otherwise MOVE it to max(q* - 1, 0).  A
 * background search of a locked slot that has seen `patience` hops without such a run gives up.  After each of the three the search
 * state (x_prev, the spectra ring, C_q, S_d, S_x, n, cand, run) is cleared and the search rests for `rest` hops.  The delay line is
 * pushed on every hop; `aligned` is exact zeros before the first lock and then `played` of `delay` hops ago, bit for bit; the hop on
 * which a lock or a move falls already carries the new delay.
 * `state` (nele_track_state_bytes(max_streams, blocks) bytes, 256-byte aligned) holds a header and one record of
 * nele_track_stream_record_bytes(blocks) bytes per slot; nele_track_init lays it out and clears every slot, nele_track_reset clears the
 * slots with slots[b] != 0 (NULL = all).  blocks = Q in 2 .. NELE_BULK_MAX_BLOCKS; the same max_streams and blocks in every call on
 * one state: a kernel given others touches nothing.
 * nele_track_set_delay: the slots with slots[b] != 0 (NULL = all) are locked at delay_hops[b] in 0 .. blocks - 1 (out of range: the slot
 *   stays as it is) and their background search starts from a cleared state, awake; delay line, counters and hop count are kept.
 * nele_track_hop: mic / played / aligned [max_streams][nh * 256] float32, hop h of the call in columns [256 h, 256 h + 256).  active
 *   [max_streams] (bytes, NULL = all): inactive slots are neither read nor written and their columns of aligned are left as they were.
 *   lambda in (0, 1), ratio > 1, hold >= 1 as for nele_bulk_hop; patience >= 1, rest >= 0 (128 and 0 are the values the search was tried
 *   with).  moved [max_streams] (bytes, or NULL) is written by every call: 1 for an active slot in which at least one move (not a first
 *   lock) fell during this call, 0 for every other slot - the `slots` argument of the next stage's reset, with no host read-back.  A
 *   slot's outputs, delay, counters and state are the same bits whatever nh per call, max_streams and the other slots are.
 * nele_track_status: info [max_streams][NELE_TRACK_INFO] int (or NULL): per slot NELE_TRACK_I_*; energies [max_streams][blocks] and conf
 *   [max_streams] float64 (or NULL): e_q and conf of the last hop a search of the slot evaluated (a clear leaves them; zeros after reset).
 * Bad host arguments are -1 before any GPU call; the *_bytes functions return -1 on bad arguments and make no HIP call.  Nothing is
 * allocated; there is no workspace. */
#define NELE_TRACK_INFO 8              /* ints per slot in nele_track_status's info */
#define NELE_TRACK_I_DELAY 0           /* hops, -1 before the first lock */
#define NELE_TRACK_I_HOPS 1            /* hops the slot has seen */
#define NELE_TRACK_I_AGE 2             /* hops the current background search has seen */
#define NELE_TRACK_I_SLEEP 3           /* hops left to rest */
#define NELE_TRACK_I_MOVES 4
#define NELE_TRACK_I_CONFIRMS 5
#define NELE_TRACK_I_GAVEUPS 6
#define NELE_TRACK_I_LAST_MOVE 7       /* the slot's hop index of the last move, -1 if none */
long long nele_track_state_bytes(int max_streams, int blocks);
long long nele_track_stream_record_bytes(int blocks);
int nele_track_init(void* state, long long state_bytes, int max_streams, int blocks, void* stream);
int nele_track_reset(void* state, long long state_bytes, int max_streams, int blocks, const unsigned char* slots, void* stream);
int nele_track_set_delay(void* state, long long state_bytes, int max_streams, int blocks, const unsigned char* slots,
                         const int* delay_hops, void* stream);
int nele_track_hop(void* state, long long state_bytes, int max_streams, int blocks, const float* mic, const float* played,
                   const unsigned char* active, int nh, double lambda, double ratio, int hold, int patience, int rest, float* aligned,
                   unsigned char* moved, void* stream);
int nele_track_status(const void* state, long long state_bytes, int max_streams, int blocks, int* info, double* energies, double* conf,
                      void* stream);

/* ---- residual-echo suppression behind the echo canceller (csrc/res.hip) ---------------------------------------------------------------
 * Per stream slot: a spectral post-filter on nele_aec_hop's residual e, driven by the canceller's own echo estimate y (DESIGN.md
 * section 17 is the arithmetic).  Per 256-sample hop, on sqrt-Hann windowed 512-sample frames [previous hop, this hop] in float64:
 * E = rfft(w e), Y = rfft(w y); S_ee, S_yy, S_ey are |E|^2, |Y|^2 and E conj(Y) smoothed by NELE_RES_SMOOTH;
 * R = |S_ey|^2 / (S_yy + NELE_RES_EPS) is the part of the residual's power that is coherent with the echo estimate,
 * G = sqrt(max(1 - beta R / (S_ee + NELE_RES_EPS), gmin^2)); out = overlap-add of w irfft(G E).  The output of hop h is the suppressed
 * residual of hop h - 1 (one hop, 16 ms, of latency; a slot's first hop is its zero history: zeros to the transforms' rounding).
 * `state` (nele_res_state_bytes(max_streams) bytes, 256-byte aligned) holds a header and one record of nele_res_stream_record_bytes()
 * bytes per slot; nele_res_init lays it out and clears every slot, nele_res_reset clears the slots with slots[b] != 0 (NULL = all).
 * The same max_streams in every call on one state: a kernel given another touches nothing.
 * nele_res_hop: residual / echo / out [max_streams][nh * 256] float32, hop h of the call in columns [256 h, 256 h + 256).
 *   gains [max_streams][nh][257] float64 (or NULL): G of every hop, for monitoring and tests.  active [max_streams] (bytes, NULL =
 *   all): inactive slots are neither read nor written and their columns of out and gains are left as they were.  beta >= 0,
 *   0 < gmin <= 1 (2.0 and 0.1 are the values the filter was tried with).  A slot's outputs and state are the same bits whatever nh
 *   per call, max_streams and the other slots are.
 * Bad host arguments are -1 before any GPU call; the *_bytes functions return -1 on bad arguments and make no HIP call.  Nothing is
 * allocated; there is no workspace. */
#define NELE_RES_SMOOTH 0.9            /* S <- NELE_RES_SMOOTH S + (1 - NELE_RES_SMOOTH) (.) for S_ee, S_yy and S_ey */
#define NELE_RES_EPS 1e-10             /* absolute, in units of unnormalised 512-point power of full-scale (+-1) signals */
long long nele_res_state_bytes(int max_streams);
long long nele_res_stream_record_bytes(void);
int nele_res_init(void* state, long long state_bytes, int max_streams, void* stream);
int nele_res_reset(void* state, long long state_bytes, int max_streams, const unsigned char* slots, void* stream);
int nele_res_hop(void* state, long long state_bytes, int max_streams, const float* residual, const float* echo,
                 const unsigned char* active, int nh, double beta, double gmin, float* out, double* gains, void* stream);

#ifdef __cplusplus
}
#endif
#endif
