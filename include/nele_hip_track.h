/* libnele_hip.so -- the fourth public header of the same library.  The rule is one header per feature added after the fixed sets: the
 * 198 entry points of include/nele_hip.h, the seven of include/nele_hip_ext.h and the five of include/nele_hip_res.h are counted by
 * their tests and stay as they are; new entry points go into a header of their own, as here.  The conventions are those of nele_hip.h,
 * as include/nele_hip_res.h restates them (device pointers unless named _host, caller-owned memory, `stream` a hipStream_t passed as
 * void*, status 0 / -1 .. -5 with nele_last_error_string(), fixed-order reductions).  tools/gen_abi.py generates
 * nele_gan_amd/_abi_track.py from this file with the parser and the type map of the other three; nele_gan_amd/_lib.py binds all four.
 * None of these is a job-table operation.
 */
#ifndef NELE_HIP_TRACK_H
#define NELE_HIP_TRACK_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- a bulk-delay search that follows the delay when it moves after the lock (csrc/bulktrack.hip) -------------------------------------
 * Per stream slot: the delay line and the search of nele_bulk_* (include/nele_hip_ext.h), with the search started
 * again from a cleared state behind every lock, over and over (DESIGN.md section 18 is the arithmetic).  A background search that
 * reaches `hold` hops in a row at block q*: the first one locks the slot at max(q* - 1, 0) hops; later ones confirm the delay when
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

#ifdef __cplusplus
}
#endif
#endif
