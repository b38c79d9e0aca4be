/* libnele_hip.so -- the eleventh public header of the same library.  include/nele_hip.h, include/nele_hip_ext.h, include/nele_hip_ext2.h,
 * include/nele_hip_ext3.h, include/nele_hip_ext4.h, include/nele_hip_ext5.h, include/nele_hip_ext6.h, include/nele_hip_ext7.h,
 * include/nele_hip_ext8.h and include/nele_hip_ext9.h are each fixed at their own set of entry points (tests/test_capi_symbols.py,
 * tests/test_abi_ext_cpu.py .. tests/test_abi_ext9_cpu.py count them).  Entry points added after those go here; the conventions are those
 * of nele_hip.h (device pointers unless named _host, caller-owned memory, `stream` a hipStream_t passed as void*, status 0 / -1 .. -5 with
 * nele_last_error_string()).  tools/gen_abi.py generates nele_gan_amd/_abi_ext10.py from this file as it generates the other ten;
 * nele_gan_amd/_lib.py binds all eleven.  None of these is a job-table operation.
 * So far: the running ESTOI of the real-time path, per stream (nele_mon_*).
 */
#ifndef NELE_HIP_EXT10_H
#define NELE_HIP_EXT10_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- running ESTOI, many concurrent streams (csrc/monitor.hip) ---------------------------------------------------
 * Per slot two time-aligned 16 kHz signals, NELE_MON_HOP samples per hop: r = `ref` of `lag` hops ago and y = `deg` of this hop (null:
 * r itself) plus `add` (null: nothing), summed in float64.  A slot's first `lag` hops only enter the history of `ref`; the measure
 * starts with hop `lag`.  All arithmetic float64:
 *   resampling  16 -> 10 kHz with ESTOI's filter (581 taps, up 5 / down 8, what scipy.signal.resample_poly(x, 5, 8, window=h) computes):
 *               output m is final once input floor((8 m + 290) / 5) has arrived, so measured hop t makes outputs 160 t - 36 ..
 *               160 t + 123 (0 .. 123 on the first), each equal to the offline resampling of the whole stream.
 *   frames      256 at hop 128, window hanning(258)[1:-1]; en_j = 20 log10(||w r_j|| + eps); M_j = max of the finite en_0 .. en_j since
 *               the slot's start or reset; frame j is kept iff en_j is finite and M_j - 40 - en_j < 0.  0, 1 or 2 frames per hop.
 *   re-analysis the windowed kept frames of both signals are overlap-added at hop 128 (zeros before the first); kept position i of that
 *               signal - it needs kept frames i - 1, i and i + 1, so it is formed when kept frame i + 1 arrives - is windowed again,
 *               transformed (512 points) and reduced to the 15 third-octave band magnitudes from 150 Hz, which enter a ring of the
 *               last 30 band vectors per signal.
 *   segment     every band vector from the 30th on: row- then column- mean/variance normalisation of both 15 x 30 blocks (oldest
 *               column first), d = sum(xn * yn) / 30.  A finite d is counted: count += 1, sum += d, last = d, smoothed += alpha (d -
 *               smoothed) (smoothed = d on the first).  Any other d is skipped: skipped += 1 and nothing else.
 *   state    one caller-owned allocation of nele_mon_state_bytes(max_streams) bytes, 256-byte aligned: a 256-byte header (max_streams,
 *            the record's bytes, lag, NELE_MON_STATS), the tables nele_mon_init computes from byte 256 (the filter by phase, float64
 *            [5][120], tap p + 5 m at [p][m]; the frame window, float64 [256], from byte 5120; the transform's twiddles, float64
 *            [256][2], from byte 7168), then from byte 11264 one record of nele_mon_stream_record_bytes() = 22272 bytes per slot:
 *              byte 0      int32 [8]: hops of ref taken while fewer than lag, the history's next place, 1 once measuring, 10 kHz samples
 *                          carried (< 256), kept frames seen (stops at 2), band vectors in the ring (stops at 30), the ring's next place,
 *                          1 once M is set
 *              byte 64     float64 [NELE_MON_STATS]: the readings below
 *              byte 256    float64 [2][128]: the last 128 samples of r and y at 16 kHz
 *              byte 2304   float64 [2][256]: the carried 10 kHz samples of r and y
 *              byte 6400   float64 [2][128]: the first half of the next re-analysis frame, overlap-added
 *              byte 8448   float64 [2][128]: the second half of the last windowed kept frame
 *              byte 10496  float64 [2][30][16]: the ring, 15 bands per place
 *              byte 18176  float32 [NELE_MON_MAX_LAG][256]: the last hops of ref
 *            Records are all zero after init or reset.  lag is fixed at init: a kernel given a state of another geometry touches nothing.
 *   ref, deg, add  [max_streams][nh * NELE_MON_HOP] float32; deg and add may be null.  active [max_streams] bytes or null (all): a slot
 *            with active[b] == 0 is neither read nor written - its state and its rows of stats, seg and nseg stay as they are.
 *   alpha    in (0, 1].
 *   stats    [max_streams][NELE_MON_STATS] float64 or null, after the call's last hop: segments counted, sum of d, last d, smoothed d,
 *            segments skipped, frames seen, frames kept, M (-inf before the first finite frame).  sum / count is the ESTOI so far.
 *   seg      [max_streams][nh][2] float64 or null: the d of the segments formed in that hop, in order (NaN for a skipped one), NaN elsewhere.
 *   nseg     [max_streams][nh] int32 or null: segments formed in that hop, counted or skipped (0 .. 2).
 * One launch per call.  A slot's outputs and state are the same bits whatever nh per call, max_streams and the other slots are.
 * Bad host arguments are -1 with the function's name before any GPU call; the *_bytes functions make no HIP call (-1 for a bad
 * argument).  Nothing is allocated. */
#define NELE_MON_HOP 256               /* samples per hop */
#define NELE_MON_STATS 8               /* doubles per stream in stats */
#define NELE_MON_MAX_LAG 4             /* hops of ref a record keeps */
long long nele_mon_state_bytes(int max_streams);
long long nele_mon_stream_record_bytes(void);
int nele_mon_init(void* state, long long state_bytes, int max_streams, int lag, void* stream);
int nele_mon_reset(void* state, long long state_bytes, int max_streams, const unsigned char* slots, void* stream);
int nele_mon_hop(void* state, long long state_bytes, int max_streams, const float* ref, const float* deg, const float* add,
                 const unsigned char* active, int nh, double alpha, double* stats, double* seg, int* nseg, void* stream);

#ifdef __cplusplus
}
#endif
#endif
