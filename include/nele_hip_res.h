/* libnele_hip.so -- the third public header of the same library.  The rule is one header per feature added after the fixed sets: the
 * 198 entry points of include/nele_hip.h are counted by its tests and the job-table operation ids of csrc/plan_ops.inc derive from
 * them, and include/nele_hip_ext.h is pinned to the bulk-delay search's seven in the same way (its opening comment still says that
 * new entry points go there; they go into a header of their own, as here).  The conventions are those of nele_hip.h (device pointers
 * unless named _host, caller-owned memory, `stream` a hipStream_t passed as void*, status 0 / -1 .. -5 with nele_last_error_string(),
 * fixed-order reductions).  tools/gen_abi.py generates nele_gan_amd/_abi_res.py from this file with the parser and the type map of the
 * other two; nele_gan_amd/_lib.py binds all three.  None of these is a job-table operation.
 */
#ifndef NELE_HIP_RES_H
#define NELE_HIP_RES_H
#ifdef __cplusplus
extern "C" {
#endif

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
