// Stream-rate conversion for the real-time path (nele_resample_stream_*): the polyphase resampler of csrc/resample.hip hop by hop on many
// concurrent streams, so that RealtimeEnhancer / EchoCanceller (16 kHz, 256-sample hops) can serve 8 .. 96 kHz devices.  The arithmetic is
// DESIGN.md section 15; tests/streamrate_ref.py restates it in numpy.  Section 12's up, down, half, table hp[up][K] and
//   y[n] = (float) sum_{k < K} hp[p][k] x[q - k],  c = n down + half,  p = c mod up,  q = c div up        (float64, k ascending, one fma per term)
// hold unchanged.  With D = half div down and r0 = half - D down (0 <= r0 < down), output m of a stream is y[m - D]: relative to the start
// of a call of nh hops (nh n_in inputs, nh n_out outputs, n_in up = n_out down) output j has c_rel = r0 + j down >= 0 and reads
// x[c_rel div up - k] of the call's row, the K - 1 samples before the row from the slot's record.  No index grows with the stream's age.
//   rss_hop_kernel   : one workgroup per stream and call, looping over the call's tiles of 256 outputs, a lane per output; per tile the
//                      input span goes to LDS as float64 beside the table and a lane runs resample_kernel<true>'s K fused multiply-adds
//                      (rs_dot of csrc/resample_poly.h, which also holds the limits and the filter's geometry for both files).
//                      The record (the last K - 1 samples of history + row, float32) is rewritten once, behind the last tile.
// State is read and written with plain loads and stores by the stream's own workgroup; no atomics, nothing crosses workgroups (a grid of
// (stream, tile) would let one workgroup overwrite the history another still reads).
#include "common.h"
#include "resample_poly.h"
#include "slot_state.h"
#include "../../include/nele_hip.h"

namespace {

constexpr long long RSS_HDR_BYTES = SLOT_GEOM_HDR_BYTES;   // int [0] = max_streams, [1] = K, [2] = up, [3] = down
__host__ __device__ constexpr long long rss_rec_bytes(int K) { return K <= 1 ? 256 : slot_al(4LL * (K - 1)); }   // float [K - 1]

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

__global__ __launch_bounds__(RS_TILE) void rss_hop_kernel(RssArgs a) {
    extern __shared__ double rss_lds[];                    // xs[span], then the table [up][K]
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= a.S) return;
    if (a.active && !a.active[b]) return;                  // neither read nor written
    if (!slot_hdr_matches(a.state, a.S, a.K, a.up, a.down)) return;   // not the state _init laid out: touch nothing
    const int K = a.K, H = K - 1, up = a.up, down = a.down;
    float* hist = reinterpret_cast<float*>(a.state + RSS_HDR_BYTES + (size_t)b * rss_rec_bytes(K));   // x[-H .. -1] of the call's row
    const float* xr = a.x + (size_t)b * a.x_stride;
    float* yr = a.y + (size_t)b * a.y_stride;
    double* xs = rss_lds;
    double* tab = rss_lds + a.span;
    for (int i = t; i < up * K; i += RS_TILE) tab[i] = a.hp[i];
    const int tiles = (a.n_out + RS_TILE - 1) / RS_TILE;
    for (int tile = 0; tile < tiles; ++tile) {
        const int j0 = tile * RS_TILE;
        const int base = (int)((a.r0 + (long long)j0 * down) / up) - H;          // xs[i] = x[base + i], base >= -H
        for (int i = t; i < a.span; i += RS_TILE) {
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
            yr[j] = (float)rs_dot(hrow, xq, K);
        }
        __syncthreads();                                   // xs is the next tile's (and the history's) staging space
    }
    float* hs = reinterpret_cast<float*>(xs);              // H floats <= span doubles
    for (int i = t; i < H; i += RS_TILE) {
        const int g = a.n_in - H + i;                      // the last H samples of history + row
        hs[i] = g < 0 ? hist[H + g] : xr[g];
    }
    __syncthreads();
    for (int i = t; i < H; i += RS_TILE) hist[i] = hs[i];
}

inline bool rss_K_ok(int K) { return K >= 1 && K <= RS_TAB_LDS_BYTES / 8; }

int rss_check(const char* name, const void* state, long long state_bytes, int S, int up, int down, int K, int* zeros) {
    if (int st = rs_check_ratio(name, up, down)) return st;
    auto params = [&]() -> int {
        *zeros = rss_K_ok(K) ? rs_zeros_of(up, down, K) : 0;
        NELE_CHECK_ARG(*zeros, "%s: K=%d is not the table width of up=%d, down=%d for any zeros in 1 .. %d", name, K, up, down, RS_MAX_ZEROS);
        NELE_CHECK_ARG((long long)up * K * 8 <= RS_TAB_LDS_BYTES, "%s: the table of up=%d, K=%d is %lld bytes, above the %d a stream converter takes",
                       name, up, K, (long long)up * K * 8, RS_TAB_LDS_BYTES);
        return NELE_OK;
    };
    return slot_state_check(name, state, state_bytes, S, params, nele_resample_stream_state_bytes(S, K), "nele_resample_stream_state_bytes", K);
}

// slots == null: every record; write_hdr: the header too
int rss_reset(const char* name, void* state, int S, int up, int down, int K, const unsigned char* slots, bool write_hdr, void* stream) {
    const int hdr[4] = {S, K, up, down};
    return slot_state_reset(name, state, RSS_HDR_BYTES, rss_rec_bytes(K), S, slots, write_hdr ? 4 : 0, hdr, stream);
}

}  // namespace

// ============================================================================================ C ABI
extern "C" int nele_resample_stream_delay(int up, int down, int zeros) {
    const char* name = "nele_resample_stream_delay";
    if (rs_check_ratio(name, up, down)) return -1;
    if (zeros < 1 || zeros > RS_MAX_ZEROS) {
        nele_set_error(NELE_ERR_INVALID_ARG, "%s: zeros=%d outside 1 .. %d", name, zeros, RS_MAX_ZEROS);
        return -1;
    }
    const int half = rs_half(up, down, zeros);
    const long long tab = (long long)up * rs_K(up, half) * 8;
    if (tab > RS_TAB_LDS_BYTES) {
        nele_set_error(NELE_ERR_INVALID_ARG, "%s: the table of up=%d, down=%d, zeros=%d is %lld bytes, above the %d a stream converter takes", name, up,
                       down, zeros, tab, RS_TAB_LDS_BYTES);
        return -1;
    }
    return half / down;
}

extern "C" int nele_resample_stream_hop_lengths(int up, int down, int to16k, int* n_in, int* n_out) {
    const char* name = "nele_resample_stream_hop_lengths";
    if (rs_check_ratio(name, up, down)) return -1;
    NELE_CHECK_ARG(n_in && n_out, "%s: null n_in or n_out", name);
    // n_in up = n_out down with 256 samples on the 16 kHz side
    const long long num = to16k ? (long long)RS_TILE * down : (long long)RS_TILE * up, den = to16k ? up : down;
    NELE_CHECK_ARG(num % den == 0,
                   "%s: a hop of 256 samples at 16 kHz is %.4f samples at the other rate (up=%d, down=%d), not a whole number: such rates "
                   "(44.1 kHz and its family) are converted offline, by nele_resample_var / python -m nele_gan_amd.resample",
                   name, (double)num / (double)den, up, down);
    *n_in = to16k ? (int)(num / den) : RS_TILE;
    *n_out = to16k ? RS_TILE : (int)(num / den);
    return NELE_OK;
}

extern "C" long long nele_resample_stream_record_bytes(int K) {
    if (!rss_K_ok(K)) return -1;
    return rss_rec_bytes(K);
}

extern "C" long long nele_resample_stream_state_bytes(int max_streams, int K) {
    if (max_streams <= 0 || max_streams > SLOT_MAX_STREAMS || !rss_K_ok(K)) return -1;
    return RSS_HDR_BYTES + (long long)max_streams * rss_rec_bytes(K);
}

extern "C" int nele_resample_stream_init(void* state, long long state_bytes, int max_streams, int up, int down, int K, void* stream) {
    int zeros = 0;
    if (int st = rss_check("nele_resample_stream_init", state, state_bytes, max_streams, up, down, K, &zeros)) return st;
    return rss_reset("nele_resample_stream_init", state, max_streams, up, down, K, nullptr, true, stream);
}

extern "C" int nele_resample_stream_reset(void* state, long long state_bytes, int max_streams, int up, int down, int K, const unsigned char* slots,
                                          void* stream) {
    int zeros = 0;
    if (int st = rss_check("nele_resample_stream_reset", state, state_bytes, max_streams, up, down, K, &zeros)) return st;
    return rss_reset("nele_resample_stream_reset", state, max_streams, up, down, K, slots, false, stream);
}

extern "C" int nele_resample_stream_hop(void* state, long long state_bytes, int max_streams, int up, int down, int K, const double* hp_dev,
                                        const float* x, long long x_stride, const unsigned char* active, int nh, int n_in_hop, float* y,
                                        long long y_stride, void* stream) {
    const char* name = "nele_resample_stream_hop";
    int zeros = 0;
    if (int st = rss_check(name, state, state_bytes, max_streams, up, down, K, &zeros)) return st;
    NELE_CHECK_ARG(hp_dev && x && y, "%s: null table, input or output", name);
    NELE_CHECK_ARG(nh >= 1 && nh <= (1 << 20), "%s: nh=%d must be in 1 .. 1048576", name, nh);
    NELE_CHECK_ARG(n_in_hop >= 1 && n_in_hop <= NELE_RESAMPLE_MAX_SAMPLES && ((long long)n_in_hop * up) % down == 0,
                   "%s: n_in_hop=%d is not a positive number of samples that up=%d / down=%d turns into a whole number", name, n_in_hop, up, down);
    const long long n_out_hop = (long long)n_in_hop * up / down, n_in = (long long)nh * n_in_hop, n_out = (long long)nh * n_out_hop;
    NELE_CHECK_ARG(n_in <= NELE_RESAMPLE_MAX_SAMPLES && n_out <= NELE_RESAMPLE_MAX_SAMPLES, "%s: nh=%d hops of %d -> %lld samples are more than 2^30 per call", name, nh, n_in_hop,
                   n_out_hop);
    const int half = rs_half(up, down, zeros), D = half / down;
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
    a.span = rs_span(up, down, K);
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
              hipLaunchKernelGGL(rss_hop_kernel, dim3(max_streams), dim3(RS_TILE), lds, as_stream(stream), a));
    NELE_CHECK_LAUNCH(name);
    return NELE_OK;
}
