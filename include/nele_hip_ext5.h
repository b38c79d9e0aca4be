/* libnele_hip.so -- the sixth public header of the same library.  include/nele_hip.h, include/nele_hip_ext.h, include/nele_hip_ext2.h,
 * include/nele_hip_ext3.h and include/nele_hip_ext4.h are each fixed at their own set of entry points (tests/test_capi_symbols.py,
 * tests/test_abi_ext_cpu.py .. tests/test_abi_ext4_cpu.py count them).  Entry points added after those go here; the conventions are
 * those of nele_hip.h (device pointers unless named _host, caller-owned memory, `stream` a hipStream_t passed as void*, status 0 /
 * -1 .. -5 with nele_last_error_string()).  tools/gen_abi.py generates nele_gan_amd/_abi_ext5.py from this file as it generates the
 * other five; nele_gan_amd/_lib.py binds all six.  None of these is a job-table operation.
 * So far: the training-free, noise-adaptive enhancer - SII-optimal band gains (nele_siiopt_mask, nele_rt_rule_*).
 */
#ifndef NELE_HIP_EXT5_H
#define NELE_HIP_EXT5_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- SII-optimal band gains (csrc/siiopt.h, csrc/siiopt.hip, csrc/realtime.hip) --------------------------------
 * Per frame the speech energy is redistributed over the 64 bands so that an approximated Speech Intelligibility Index is maximal at
 * unchanged total power (Taal, Jensen & Leijon, IEEE SPL 2013): closed-form water-filling on the long-term speech band powers and the
 * noise band powers - the generator's own two inputs - and a mask in the generator's own range.  float64 throughout:
 *   P = (double)cb ** 6;  N = max((double)nb ** 6, NELE_SIIOPT_NMIN) (a NaN feature gives the floor)
 *   Sbar += max(1 / (t + 1), 1 - lam) (P - Sbar)                                  frame t = 0, 1, .. of the row or stream, per band
 *   r = sum Sbar;  active = {gamma > 0 and Sbar > 0};  repeat  c = (r + sum_act N) / sum_act sqrt(gamma N),
 *     p = c sqrt(gamma N) - N,  drop the active bands with p <= 0  until none is dropped;  p = 0 off the active set
 *   alpha = Sbar > 0 ? p / Sbar : 1, clamped to exp(-+NELE_SIIOPT_LOGMAX);  mask = float32(strength == 1 ? alpha : alpha ** strength)
 * gamma [64] float64 >= 0 (band importance), 0 <= lam < 1, 0 < strength <= 1.  A row's or slot's mask is the same bits whatever B, its
 * position, the hop grouping and the other rows are, and the same bits offline and streamed.
 * nele_siiopt_mask: cb, nb, mask [B][T][64] float32 (the layouts of the generator's forward pass); no workspace.
 * nele_rt_rule_hop / nele_rt_rule_finish: nele_rt_hop / nele_rt_finish (nele_hip.h) with the rule in the generator's place - the same
 *   state buffer, laid out by nele_rt_state_bytes and initialised by nele_rt_reset alone (the weights area is never read), the same
 *   arguments without `precision`, the same outputs.  Two launches per hop.  The only state the rule adds is Sbar [64] float64 per
 *   stream, kept in the record where the generator's first history ring lies: a state buffer serves one of the two modes between resets.
 * Bad host arguments are -1 with the function's name before any GPU call.  Nothing is allocated. */
#define NELE_SIIOPT_LAMBDA 0.98        /* default lam: the long-term speech power forgets with a time constant of 50 frames (0.8 s) */
#define NELE_SIIOPT_NMIN 1e-30         /* floor of the noise band power */
#define NELE_SIIOPT_LOGMAX 3.2         /* |log mask| <= this: the generator's own mask range exp(3.2 tanh) */
int nele_siiopt_mask(const float* cb, const float* nb, const double* gamma, int B, int T, double lam, double strength, float* mask,
                     void* stream);
int nele_rt_rule_hop(void* state, long long state_bytes, int max_streams, const double* gamma, double lam, double strength,
                     const float* clean, const float* noise, const unsigned char* active, int nh, const float* beta2, float* out,
                     float* dbg_band, float* dbg_noise, float* dbg_mask, float* dbg_alpha2, int dbg_frames, void* stream);
int nele_rt_rule_finish(void* state, long long state_bytes, int max_streams, const double* gamma, double lam, double strength,
                        const float* clean_tail, const float* noise_tail, const int* tail_lengths, const float* beta2, float* out,
                        float* dbg_band, float* dbg_noise, float* dbg_mask, float* dbg_alpha2, int dbg_frames, void* stream);

#ifdef __cplusplus
}
#endif
#endif
