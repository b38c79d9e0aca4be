/* libnele_hip.so -- the fifth public header of the same library.  include/nele_hip.h, include/nele_hip_ext.h, include/nele_hip_ext2.h
 * and include/nele_hip_ext3.h are each fixed at their own set of entry points (tests/test_capi_symbols.py, tests/test_abi_ext_cpu.py,
 * tests/test_abi_ext2_cpu.py and tests/test_abi_ext3_cpu.py count them).  Entry points added after those go here; the conventions are
 * those of nele_hip.h (device pointers unless named _host, caller-owned memory, `stream` a hipStream_t passed as void*, status 0 /
 * -1 .. -5 with nele_last_error_string()).  tools/gen_abi.py generates nele_gan_amd/_abi_ext4.py from this file as it generates the
 * other four; nele_gan_amd/_lib.py binds all five.  None of these is a job-table operation.
 * So far: the near-end noise suppressor of the real-time uplink (nele_ns_*).
 */
#ifndef NELE_HIP_EXT4_H
#define NELE_HIP_EXT4_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- noise suppression for the uplink (csrc/ns.hip) ---------------------------------------------------------------
 * What the echo canceller leaves is the near-end talker plus the room's noise; this takes the noise out of it: the optimally-modified
 * log-spectral amplitude gain (Cohen & Berdugo 2001) on the project's IMCRA noise tracker, on the real-time path's blocks - 256-sample
 * hops, sqrt-Hann 512-sample frames, float64 transforms.  Per hop and slot:
 *   E = rfft512(w [x_prev, x]);  Y2f = float32(|E|^2 + NELE_NS_EPS);  one IMCRA frame on Y2f (speech-presence probability p uncapped)
 *   nu = Gamma xi / (1 + xi);  G_H1 = min(xi / (1 + xi) exp(E1(max(nu, NELE_NS_NU_MIN)) / 2), 1);  G = exp(p ln G_H1 + (1 - p) ln gmin)
 *   out = float32(ola + o[0:256]), ola <- o[256:512], o = w irfft512(G E):  the output is ONE HOP LATE.
 * The first 15 frames of a slot (240 ms) have G = gmin: IMCRA takes them as noise.
 * `state` (nele_ns_state_bytes(max_streams) bytes, 256-byte aligned): a 256-byte header (max_streams, the record's bytes), then one
 *   record of nele_ns_stream_record_bytes() bytes per slot (the frame counters, x_prev, the overlap-add tail, IMCRA's per-bin state and
 *   its two eight-slot minima rings).  nele_ns_init lays it out and zeroes every record; nele_ns_reset zeroes the records of the slots
 *   with slots[b] != 0 (NULL = all).  A kernel given a state laid out for another max_streams touches nothing.
 * nele_ns_hop: x, out [max_streams][nh * 256] float32; gmin in (0, 1]; gains, noise_psd, presence [max_streams][nh][257] float64 or
 *   NULL each: G, lambda_D after the frame, p.  active [max_streams] (bytes, NULL = all): inactive slots are neither read nor written
 *   and their columns of the outputs are left as they were.  A slot's outputs and state are the same bits whatever nh per call,
 *   max_streams and the other slots.
 * Bad host arguments are -1 before any GPU call; the *_bytes functions return -1 on bad arguments and make no HIP call.  Nothing is
 * allocated; there is no workspace. */
#define NELE_NS_EPS 1e-10              /* added to |E|^2: lets a stream start on digital silence */
#define NELE_NS_NU_MIN 1e-8            /* floor of E1's argument */
long long nele_ns_state_bytes(int max_streams);
long long nele_ns_stream_record_bytes(void);
int nele_ns_init(void* state, long long state_bytes, int max_streams, void* stream);
int nele_ns_reset(void* state, long long state_bytes, int max_streams, const unsigned char* slots, void* stream);
int nele_ns_hop(void* state, long long state_bytes, int max_streams, const float* x, const unsigned char* active, int nh, double gmin,
                float* out, double* gains, double* noise_psd, double* presence, void* stream);

#ifdef __cplusplus
}
#endif
#endif
