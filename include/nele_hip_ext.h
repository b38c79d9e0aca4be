/* libnele_hip.so -- the second public header of the same library: entry points added after the 198 of include/nele_hip.h, whose set is
 * fixed (its tests count them and the job-table operation ids of csrc/plan_ops.inc derive from it).  New entry points go here; the
 * conventions are those of nele_hip.h (device pointers unless named _host, caller-owned memory, `stream` a hipStream_t passed as void*,
 * status 0 / -1 .. -5 with nele_last_error_string(), fixed-order reductions).  tools/gen_abi.py generates nele_gan_amd/_abi_ext.py from
 * this file as it generates _abi.py from nele_hip.h; nele_gan_amd/_lib.py binds both.  None of these is a job-table operation.
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

#ifdef __cplusplus
}
#endif
#endif
