// Stream-rate conversion for the real-time path (nele_resample_stream_*): the polyphase resampler of csrc/resample.hip hop by hop on many
// concurrent streams, so that RealtimeEnhancer / EchoCanceller (16 kHz, 256-sample hops) can serve 8 .. 96 kHz devices.  The arithmetic is
// DESIGN.md section 15; tests/streamrate_ref.py restates it in numpy.  Section 12's up, down, half, table hp[up][K] and
//   y[n] = (float) sum_{k < K} hp[p][k] x[q - k],  c = n down + half,  p = c mod up,  q = c div up        (float64, k ascending, one fma per term)
// hold unchanged.  With D = half div down and r0 = half - D down (0 <= r0 < down), output m of a stream is y[m - D]: relative to the start
// of a call of nh hops (nh n_in inputs, nh n_out outputs, n_in up = n_out down) output j has c_rel = r0 + j down >= 0 and reads
// x[c_rel div up - k] of the call's row, the K - 1 samples before the row from the slot's record.  No index grows with the stream's age.
//   rss_hop_kernel   : one workgroup per stream and call, looping over the call's tiles of 256 outputs, a lane per output; per tile the
//                      input span goes to LDS as float64 beside the table and a lane runs resample_kernel<true>'s K fused multiply-adds.
//                      The record (the last K - 1 samples of history + row, float32) is rewritten once, behind the last tile.
//   rss_reset_kernel : zeroes the records of the chosen slots
// State is read and written with plain loads and stores by the stream's own workgroup; no atomics, nothing crosses workgroups (a grid of
// (stream, tile) would let one workgroup overwrite the history another still reads).
#include "common.h"
#include "../../include/nele_hip.h"

namespace {

#define RSS_TILE 256                   // outputs per tile = threads per workgroup
#define RSS_TAB_LDS_BYTES 16384        // the table must fit the LDS form of csrc/resample.hip
#define RSS_MAX_RATIO 16               // the limits of nele_resample_var (csrc/resample.hip)
#define RSS_MAX_FACTOR 1024
#define RSS_MAX_ZEROS 64
#define RSS_MAX_CALL (1 << 30)         // input and output samples per row and call
constexpr long long RSS_HDR_BYTES = 256;                   // int [0] = max_streams, [1] = K, [2] = up, [3] = down
__host__ __device__ constexpr long long rss_rec_bytes(int K) { return K <= 1 ? 256 : (4LL * (K - 1) + 255) / 256 * 256; }   // float [K - 1]
// input samples a tile can touch (as rs_span of csrc/resample.hip): q_last - q_first <= floor(255 down / up) + 1, K - 1 in front
__host__ __device__ inline int rss_span(int up, int down, int K) { return (int)(((long long)(RSS_TILE - 1) * down) / up) + K + 1; }

struct RssArgs {
    unsigned char* state;
    int S, up, down, K;
    int r0;                      // half - D down: c_rel of the call's first output
    int span;
    int n_in, n_out;             // samples per row in this call
    const double* hp;            // [up][K]
    const float* x;              // [S] rows of x_stride
    long long x_stride;
    const unsigned char* active; // [S] or null (all)
    float* y;                    // [S] rows of y_stride
    long long y_stride;
};

__global__ __launch_bounds__(RSS_TILE) void rss_hop_kernel(RssArgs a) {
    extern __shared__ double rss_lds[];                    // xs[span], then the table [up][K]
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= a.S) return;
    if (a.active && !a.active[b]) return;                  // neither read nor written
    const int* hdr = reinterpret_cast<const int*>(a.state);
    if (hdr[0] != a.S || hdr[1] != a.K || hdr[2] != a.up || hdr[3] != a.down) return;       // not the state _init laid out: touch nothing
    const int K = a.K, H = K - 1, up = a.up, down = a.down;
    float* hist = reinterpret_cast<float*>(a.state + RSS_HDR_BYTES + (size_t)b * rss_rec_bytes(K));   // x[-H .. -1] of the call's row
    const float* xr = a.x + (size_t)b * a.x_stride;
    float* yr = a.y + (size_t)b * a.y_stride;
    double* xs = rss_lds;
    double* tab = rss_lds + a.span;
    for (int i = t; i < up * K; i += RSS_TILE) tab[i] = a.hp[i];
    const int tiles = (a.n_out + RSS_TILE - 1) / RSS_TILE;
    for (int tile = 0; tile < tiles; ++tile) {
        const int j0 = tile * RSS_TILE;
        const int base = (int)((a.r0 + (long long)j0 * down) / up) - H;          // xs[i] = x[base + i], base >= -H
        for (int i = t; i < a.span; i += RSS_TILE) {
            const int g = base + i;
            xs[i] = g < 0 ? (double)hist[H + g] : (g < a.n_in ? (double)xr[g] : 0.0);
        }
        __syncthreads();
        const int j = j0 + t;
        if (j < a.n_out) {
            const long long c = a.r0 + (long long)j * down;
            const int p = (int)(c % up);
            const double* __restrict__ hrow = tab + (size_t)p * K;
            const double* __restrict__ xq = xs + ((int)(c / up) - base);       // x[q]; x[q - k] = xq[-k], 0 <= index < span
            double acc = 0.0;
#pragma unroll 8
            for (int k = 0; k < K; ++k) acc = fma(hrow[k], xq[-k], acc);
            yr[j] = (float)acc;
        }
        __syncthreads();                                   // xs is the next tile's (and the history's) staging space
    }
    float* hs = reinterpret_cast<float*>(xs);              // H floats <= span doubles
    for (int i = t; i < H; i += RSS_TILE) {
        const int g = a.n_in - H + i;                      // the last H samples of history + row
        hs[i] = g < 0 ? hist[H + g] : xr[g];
    }
    __syncthreads();
    for (int i = t; i < H; i += RSS_TILE) hist[i] = hs[i];
}

// slots == null: every record; write_hdr: the header too
__global__ void rss_reset_kernel(unsigned char* __restrict__ state, int S, int K, int up, int down, const unsigned char* __restrict__ slots,
                                 int write_hdr) {
    const int b = blockIdx.x;
    if (write_hdr && b == 0 && threadIdx.x < RSS_HDR_BYTES / 4) {
        int* hdr = reinterpret_cast<int*>(state);
        const int v[4] = {S, K, up, down};
        hdr[threadIdx.x] = threadIdx.x < 4 ? v[threadIdx.x] : 0;
    }
    if (b >= S || (slots && !slots[b])) return;
    const long long rb = rss_rec_bytes(K);
    uint4* r = reinterpret_cast<uint4*>(state + RSS_HDR_BYTES + (size_t)b * rb);
    for (long long i = threadIdx.x; i < rb / 16; i += blockDim.x) r[i] = make_uint4(0u, 0u, 0u, 0u);
}

inline int rss_half(int up, int down, int zeros) { return zeros * (up > down ? up : down); }
inline int rss_K(int up, int half) { return (2 * half + 1 + up - 1) / up; }
inline bool rss_K_ok(int K) { return K >= 1 && K <= RSS_TAB_LDS_BYTES / 8; }

int rss_check_ratio(const char* name, int up, int down) {
    NELE_CHECK_ARG(up >= 1 && up <= RSS_MAX_FACTOR && down >= 1 && down <= RSS_MAX_FACTOR, "%s: up=%d or down=%d outside 1 .. %d", name, up, down,
                   RSS_MAX_FACTOR);
    NELE_CHECK_ARG(down <= RSS_MAX_RATIO * up && up <= RSS_MAX_RATIO * down, "%s: up=%d / down=%d outside 1/%d .. %d", name, up, down, RSS_MAX_RATIO,
                   RSS_MAX_RATIO);
    return NELE_OK;
}

// the zeros in 1 .. 64 whose table width is K (0: none), as nele_resample_var finds it
int rss_zeros_of(int up, int down, int K) {
    for (int z = 1; z <= RSS_MAX_ZEROS; ++z)
        if (rss_K(up, rss_half(up, down, z)) == K) return z;
    return 0;
}

int rss_check(const char* name, const void* state, long long state_bytes, int S, int up, int down, int K, int* zeros) {
    if (int st = rss_check_ratio(name, up, down)) return st;
    NELE_CHECK_ARG(state, "%s: null state", name);
    NELE_CHECK_ARG(S > 0 && S <= (1 << 20), "%s: max_streams=%d must be in 1 .. 1048576", name, S);
    *zeros = rss_K_ok(K) ? rss_zeros_of(up, down, K) : 0;
    NELE_CHECK_ARG(*zeros, "%s: K=%d is not the table width of up=%d, down=%d for any zeros in 1 .. %d", name, K, up, down, RSS_MAX_ZEROS);
    NELE_CHECK_ARG((long long)up * K * 8 <= RSS_TAB_LDS_BYTES, "%s: the table of up=%d, K=%d is %lld bytes, above the %d a stream converter takes", name,
                   up, K, (long long)up * K * 8, RSS_TAB_LDS_BYTES);
    NELE_CHECK_ARG(state_bytes >= nele_resample_stream_state_bytes(S, K),
                   "%s: state of %lld bytes is smaller than nele_resample_stream_state_bytes(%d, %d) = %lld", name, state_bytes, S, K,
                   nele_resample_stream_state_bytes(S, K));
    NELE_CHECK_ARG(((size_t)state % 256) == 0, "%s: state must be 256-byte aligned", name);
    return NELE_OK;
}

}  // namespace

// ============================================================================================ C ABI
extern "C" int nele_resample_stream_delay(int up, int down, int zeros) {
    const char* name = "nele_resample_stream_delay";
    if (rss_check_ratio(name, up, down)) return -1;
    if (zeros < 1 || zeros > RSS_MAX_ZEROS) {
        nele_set_error(NELE_ERR_INVALID_ARG, "%s: zeros=%d outside 1 .. %d", name, zeros, RSS_MAX_ZEROS);
        return -1;
    }
    const int half = rss_half(up, down, zeros);
    const long long tab = (long long)up * rss_K(up, half) * 8;
    if (tab > RSS_TAB_LDS_BYTES) {
        nele_set_error(NELE_ERR_INVALID_ARG, "%s: the table of up=%d, down=%d, zeros=%d is %lld bytes, above the %d a stream converter takes", name, up,
                       down, zeros, tab, RSS_TAB_LDS_BYTES);
        return -1;
    }
    return half / down;
}

extern "C" int nele_resample_stream_hop_lengths(int up, int down, int to16k, int* n_in, int* n_out) {
    const char* name = "nele_resample_stream_hop_lengths";
    if (rss_check_ratio(name, up, down)) return -1;
    NELE_CHECK_ARG(n_in && n_out, "%s: null n_in or n_out", name);
    // n_in up = n_out down with 256 samples on the 16 kHz side
    const long long num = to16k ? (long long)RSS_TILE * down : (long long)RSS_TILE * up, den = to16k ? up : down;
    NELE_CHECK_ARG(num % den == 0,
                   "%s: a hop of 256 samples at 16 kHz is %.4f samples at the other rate (up=%d, down=%d), not a whole number: such rates "
                   "(44.1 kHz and its family) are converted offline, by nele_resample_var / python -m nele_gan_amd.resample",
                   name, (double)num / (double)den, up, down);
    *n_in = to16k ? (int)(num / den) : RSS_TILE;
    *n_out = to16k ? RSS_TILE : (int)(num / den);
    return NELE_OK;
}

extern "C" long long nele_resample_stream_record_bytes(int K) {
    if (!rss_K_ok(K)) return -1;
    return rss_rec_bytes(K);
}

extern "C" long long nele_resample_stream_state_bytes(int max_streams, int K) {
    if (max_streams <= 0 || max_streams > (1 << 20) || !rss_K_ok(K)) return -1;
    return RSS_HDR_BYTES + (long long)max_streams * rss_rec_bytes(K);
}

extern "C" int nele_resample_stream_init(void* state, long long state_bytes, int max_streams, int up, int down, int K, void* stream) {
    int zeros = 0;
    if (int st = rss_check("nele_resample_stream_init", state, state_bytes, max_streams, up, down, K, &zeros)) return st;
    hipLaunchKernelGGL(rss_reset_kernel, dim3(max_streams), dim3(256), 0, as_stream(stream), (unsigned char*)state, max_streams, K, up, down,
                       (const unsigned char*)nullptr, 1);
    NELE_CHECK_LAUNCH("nele_resample_stream_init");
    return NELE_OK;
}

extern "C" int nele_resample_stream_reset(void* state, long long state_bytes, int max_streams, int up, int down, int K, const unsigned char* slots,
                                          void* stream) {
    int zeros = 0;
    if (int st = rss_check("nele_resample_stream_reset", state, state_bytes, max_streams, up, down, K, &zeros)) return st;
    hipLaunchKernelGGL(rss_reset_kernel, dim3(max_streams), dim3(256), 0, as_stream(stream), (unsigned char*)state, max_streams, K, up, down, slots, 0);
    NELE_CHECK_LAUNCH("nele_resample_stream_reset");
    return NELE_OK;
}

extern "C" int nele_resample_stream_hop(void* state, long long state_bytes, int max_streams, int up, int down, int K, const double* hp_dev,
                                        const float* x, long long x_stride, const unsigned char* active, int nh, int n_in_hop, float* y,
                                        long long y_stride, void* stream) {
    const char* name = "nele_resample_stream_hop";
    int zeros = 0;
    if (int st = rss_check(name, state, state_bytes, max_streams, up, down, K, &zeros)) return st;
    NELE_CHECK_ARG(hp_dev && x && y, "%s: null table, input or output", name);
    NELE_CHECK_ARG(nh >= 1 && nh <= (1 << 20), "%s: nh=%d must be in 1 .. 1048576", name, nh);
    NELE_CHECK_ARG(n_in_hop >= 1 && n_in_hop <= RSS_MAX_CALL && ((long long)n_in_hop * up) % down == 0,
                   "%s: n_in_hop=%d is not a positive number of samples that up=%d / down=%d turns into a whole number", name, n_in_hop, up, down);
    const long long n_out_hop = (long long)n_in_hop * up / down, n_in = (long long)nh * n_in_hop, n_out = (long long)nh * n_out_hop;
    NELE_CHECK_ARG(n_in <= RSS_MAX_CALL && n_out <= RSS_MAX_CALL, "%s: nh=%d hops of %d -> %lld samples are more than 2^30 per call", name, nh, n_in_hop,
                   n_out_hop);
    const int half = rss_half(up, down, zeros), D = half / down;
    NELE_CHECK_ARG(D <= n_out_hop, "%s: the delay of %d output samples is longer than a hop of %lld", name, D, n_out_hop);
    NELE_CHECK_ARG(x_stride >= n_in && y_stride >= n_out, "%s: x_stride=%lld below nh n_in_hop=%lld or y_stride=%lld below nh n_out=%lld", name, x_stride,
                   n_in, y_stride, n_out);
    RssArgs a{};
    a.state = (unsigned char*)state;
    a.S = max_streams;
    a.up = up;
    a.down = down;
    a.K = K;
    a.r0 = half - D * down;
    a.span = rss_span(up, down, K);
    a.n_in = (int)n_in;
    a.n_out = (int)n_out;
    a.hp = hp_dev;
    a.x = x;
    a.x_stride = x_stride;
    a.active = active;
    a.y = y;
    a.y_stride = y_stride;
    const size_t lds = ((size_t)a.span + (size_t)up * K) * sizeof(double);      // <= 49040 + 16384 bytes: inside the 64 KiB of a plain launch
    NELE_PROF("resample_stream", as_stream(stream),
              hipLaunchKernelGGL(rss_hop_kernel, dim3(max_streams), dim3(RSS_TILE), lds, as_stream(stream), a));
    NELE_CHECK_LAUNCH(name);
    return NELE_OK;
}
