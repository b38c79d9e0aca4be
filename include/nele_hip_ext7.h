/* libnele_hip.so -- the eighth public header of the same library.  include/nele_hip.h, include/nele_hip_ext.h, include/nele_hip_ext2.h,
 * include/nele_hip_ext3.h, include/nele_hip_ext4.h, include/nele_hip_ext5.h and include/nele_hip_ext6.h are each fixed at their own set
 * of entry points (tests/test_capi_symbols.py, tests/test_abi_ext_cpu.py .. tests/test_abi_ext6_cpu.py count them).  Entry points added
 * after those go here; the conventions are those of nele_hip.h (device pointers unless named _host, caller-owned memory, `stream` a
 * hipStream_t passed as void*, status 0 / -1 .. -5 with nele_last_error_string()).  tools/gen_abi.py generates
 * nele_gan_amd/_abi_ext7.py from this file as it generates the other seven; nele_gan_amd/_lib.py binds all eight.  None of these is a
 * job-table operation.
 * So far: the up-converter of the real-time path that carries the band above 8 kHz past the enhancer (nele_hbup_*).
 */
#ifndef NELE_HIP_EXT7_H
#define NELE_HIP_EXT7_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- 16 kHz -> device rate with the high band carried, many concurrent streams (csrc/highband.hip) -------------
 * Per stream, with zeros before its start, lam = lag16 and L = lag_dev:
 *   d[n] = fmaf(-g, low[n - lam], enh[n])                      float32, at 16 kHz
 *   u[m] = the stream up-converter's output for d              (nele_resample_stream_hop's sum: float64, k ascending, one fma per term)
 *   y[m] = fmaf(g, x[m - L], (float)u[m])                      float32, at the device rate
 * low is the down-converter's output for x, enh what the enhancer made of low lam samples earlier.  With L the delay of x through
 * down-converter, enhancer and up-converter, g (x[m - L] - up(low delayed)[m]) is the part of x the 16 kHz path cannot carry.
 *   up, down, K, hp_dev   the up-converter's ratio, table width and table [up][K] (nele_resample_taps, layout 1); 256 up must be a
 *            multiple of down: a hop of 256 samples at 16 kHz is 256 up / down samples at the device rate.
 *   state    one caller-owned allocation of nele_hbup_state_bytes(..) bytes, 256-byte aligned: a header, then one record of
 *            nele_hbup_record_bytes(..) per slot - float32: the last K - 1 of d, the last lag16 of low, the last lag_dev of x.
 *   enh, low [max_streams] rows of nh * 256 float32, enh_stride / low_stride apart; x, y [max_streams] rows of nh * 256 up / down
 *            float32, x_stride / y_stride apart; y overlaps none of the inputs.
 *   gain     [max_streams] float32, g of each slot, or null (1 for all).
 *   active   [max_streams] bytes or null (all): a slot with active[b] == 0 is neither read nor written.
 * One launch per call.  A slot's outputs and state are the same bits whatever nh per call, max_streams and the other slots are.
 * Bad host arguments are -1 with the function's name before any GPU call; the *_bytes functions make no HIP call (-1 for a bad
 * argument).  Nothing is allocated. */
#define NELE_HBUP_MAX_LAG16 2048       /* largest lag16: eight hops at 16 kHz */
#define NELE_HBUP_MAX_LAG 16384        /* largest lag_dev, in device-rate samples */
long long nele_hbup_record_bytes(int K, int lag16, int lag_dev);
long long nele_hbup_state_bytes(int max_streams, int K, int lag16, int lag_dev);
int nele_hbup_init(void* state, long long state_bytes, int max_streams, int up, int down, int K, int lag16, int lag_dev, void* stream);
int nele_hbup_reset(void* state, long long state_bytes, int max_streams, int up, int down, int K, int lag16, int lag_dev,
                    const unsigned char* slots, void* stream);
int nele_hbup_hop(void* state, long long state_bytes, int max_streams, int up, int down, int K, int lag16, int lag_dev, const double* hp_dev,
                  const float* enh, long long enh_stride, const float* low, long long low_stride, const float* x, long long x_stride,
                  const float* gain, const unsigned char* active, int nh, float* y, long long y_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif
