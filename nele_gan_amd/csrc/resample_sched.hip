// Stream-rate conversion on a hop schedule (nele_sched_stream_*): csrc/resample_stream.hip's converter for the device rates at which a
// 256-sample hop at 16 kHz is NOT a whole number of device samples - 44.1 kHz and its family - and, as the case P = 1, for the others.
// The arithmetic is DESIGN.md section 20; tests/schedrate_ref.py restates it in numpy.  Section 12's up, down, half, table hp[up][K] and
//   y[n] = (float) sum_{k < K} hp[p][k] x[q - k],  c = n down + half,  p = c mod up,  q = c div up        (float64, k ascending, one fma per term)
// hold unchanged.  The 16 kHz side moves 256 samples per hop, the device side n(g) = floor((g + 1) r) - floor(g r) at schedule position
// g, r = 256 sr_dev / 16000 = num / P.  A slot keeps H = K - 1 + E input samples and its lead L: relative to the first input sample of
// its next hop, output j has c_rel = L + j down (negative at times: hence E more samples than section 15's K - 1) and reads
// x[c_rel div up - k]; behind a call of n_in inputs and n_out outputs L <- L + n_out down - n_in up.
//   sched_hop_kernel : one workgroup per slot and call, looping over the call's tiles of 256 outputs, a lane per output.  Per tile the
//                      input span goes to LDS as float64 - from the record where the index lies before the row, from the row otherwise -
//                      and a lane runs rs_dot of csrc/resample_poly.h on its own table row: from global memory (the 220 .. 325 KiB
//                      tables of the family live in L2; a lane's row is contiguous) or, where the table is at most RS_TAB_LDS_BYTES
//                      (the P = 1 rates), from LDS beside the span.  The record is rewritten once, behind the last tile.
// State is read and written with plain loads and stores by the slot's own workgroup; no atomics, nothing crosses workgroups.
#include "common.h"
#include "resample_poly.h"
#include "slot_state.h"
#include "../../include/nele_hip.h"
#include "../../include/nele_hip_ext3.h"

namespace {

constexpr long long SCH_HDR_BYTES = SLOT_GEOM_HDR_BYTES;   // int [0] = max_streams, [1] = K, [2] = up, [3] = down, [4] = to16k, [5] = H, [6] = L0
constexpr int SCH_HEAD_BYTES = 16;                          // a record: int lead, three reserved ints, then float [H]
constexpr int SCH_MAX_H = 4096;                             // above every H the limits of section 12 allow (K <= 2049, E <= 18)
__host__ __device__ constexpr long long sch_rec_bytes(int H) { return slot_al(SCH_HEAD_BYTES + 4LL * H); }

struct SchPlan {
    int half, K, D, L0, E, H, P, hop_min, hop_max;
    long long rnum;                                         // r = rnum / P
};

long long sch_gcd(long long a, long long b) {
    while (b) {
        const long long t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// section 20: W = the swing of the lead, D = (half + W) div down, L0 = half - D down, E = max(0, ceil((W - L0) / up)), H = K - 1 + E
SchPlan sch_plan(int up, int down, int zeros, int to16k) {
    SchPlan s{};
    s.half = rs_half(up, down, zeros);
    s.K = rs_K(up, s.half);
    const long long den = to16k ? up : down, num = (long long)RS_TILE * (to16k ? down : up), g = sch_gcd(num, den);
    s.rnum = num / g;
    s.P = (int)(den / g);
    const int W = (int)(den - g);                           // up - up / P towards 16 kHz, down - down / P away from it
    s.D = (s.half + W) / down;
    s.L0 = s.half - s.D * down;
    s.E = W - s.L0 > 0 ? (W - s.L0 + up - 1) / up : 0;
    s.H = s.K - 1 + s.E;
    s.hop_min = (int)(s.rnum / s.P);
    s.hop_max = (int)((s.rnum + s.P - 1) / s.P);
    return s;
}

// the device-side samples of nh hops from position pos
long long sch_dev_width(const SchPlan& s, int pos, int nh) { return ((long long)pos + nh) * s.rnum / s.P - (long long)pos * s.rnum / s.P; }

int sch_check_plan(const char* name, int up, int down, int zeros, int to16k, SchPlan* s) {
    if (int st = rs_check_ratio(name, up, down)) return st;
    NELE_CHECK_ARG(zeros >= 1 && zeros <= RS_MAX_ZEROS, "%s: zeros=%d outside 1 .. %d", name, zeros, RS_MAX_ZEROS);
    *s = sch_plan(up, down, zeros, to16k);
    const int shortest = to16k ? RS_TILE : s->hop_min;
    NELE_CHECK_ARG(s->D <= shortest, "%s: the delay of %d output samples is longer than the shortest hop of %d (up=%d, down=%d, zeros=%d)", name, s->D,
                   shortest, up, down, zeros);
    return NELE_OK;
}

struct SchArgs {
    unsigned char* state;
    int S, up, down, K, H, E, L0, to16k;
    int span;
    int n_in, n_out;             // samples per row in this call
    const double* hp;            // [up][K]
    const float* x;              // [S] rows of x_stride
    long long x_stride;
    const unsigned char* active; // [S] or null (all)
    float* y;                    // [S] rows of y_stride
    long long y_stride;
};

template <bool TAB_LDS>
__global__ __launch_bounds__(RS_TILE) void sched_hop_kernel(SchArgs a) {
    extern __shared__ double sch_lds[];                    // xs[max(span, H / 2)], then (TAB_LDS) the table [up][K]
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= a.S) return;
    if (a.active && !a.active[b]) return;                  // neither read nor written
    if (!slot_hdr_matches(a.state, a.S, a.K, a.up, a.down, a.to16k, a.H, a.L0)) return;   // not the state _init laid out: touch nothing
    const int K = a.K, H = a.H, up = a.up, down = a.down;
    int* head = reinterpret_cast<int*>(a.state + SCH_HDR_BYTES + (size_t)b * sch_rec_bytes(H));
    float* hist = reinterpret_cast<float*>(head + SCH_HEAD_BYTES / 4);                    // buf[0 .. H) of buf = history ++ row
    const float* xr = a.x + (size_t)b * a.x_stride;
    float* yr = a.y + (size_t)b * a.y_stride;
    const int L = head[0];
    // the guard: inside these bounds every read index lies in 0 .. H + n_in - 1 of buf (the smallest is (L div up) + E >= 0, the largest
    // (L + (n_out - 1) down) div up + H < n_in + H); outside them the slot's lead is not this call's: NaN, and the record stays
    if (L < -a.E * up || (long long)L + (long long)(a.n_out - 1) * down >= (long long)a.n_in * up) {
        for (int j = t; j < a.n_out; j += RS_TILE) yr[j] = __int_as_float(0x7fc00000);
        return;
    }
    double* xs = sch_lds;
    const double* tab = a.hp;
    if (TAB_LDS) {
        double* tl = sch_lds + (a.span > (H + 1) / 2 ? a.span : (H + 1) / 2);
        for (int i = t; i < up * K; i += RS_TILE) tl[i] = a.hp[i];
        tab = tl;
    }
    const long long c0 = (long long)L + (long long)a.E * up;                              // >= 0; c0 + j down = c_rel + E up: the same phase, q + E
    const int tiles = (a.n_out + RS_TILE - 1) / RS_TILE;
    for (int tile = 0; tile < tiles; ++tile) {
        const int j0 = tile * RS_TILE;
        const int base = (int)((c0 + (long long)j0 * down) / up);                         // xs[i] = buf[base + i]; x[q - k] of output j is buf[q + K - 1 - k]
        for (int i = t; i < a.span; i += RS_TILE) {
            const int g = base + i;
            xs[i] = g < H ? (double)hist[g] : (g - H < a.n_in ? (double)xr[g - H] : 0.0);
        }
        __syncthreads();
        const int j = j0 + t;
        if (j < a.n_out) {
            const long long c = c0 + (long long)j * down;
            const int p = (int)(c % up);
            const double* __restrict__ hrow = tab + (size_t)p * K;
            const double* __restrict__ xq = xs + ((int)(c / up) - base + K - 1);          // xq[-k], 0 <= index < span
            yr[j] = (float)rs_dot(hrow, xq, K);
        }
        __syncthreads();                                   // xs is the next tile's (and the history's) staging space
    }
    float* hs = reinterpret_cast<float*>(xs);              // H floats fit: the launch sizes xs for both
    for (int i = t; i < H; i += RS_TILE) {
        const int g = a.n_in + i;                          // the last H samples of buf
        hs[i] = g < H ? hist[g] : xr[g - H];
    }
    __syncthreads();
    for (int i = t; i < H; i += RS_TILE) hist[i] = hs[i];
    if (t == 0) head[0] = (int)((long long)L + (long long)a.n_out * down - (long long)a.n_in * up);
}

struct SchGeom {
    SchPlan plan;
    int zeros;
};

int sch_check(const char* name, const void* state, long long state_bytes, int S, int up, int down, int K, int to16k, SchGeom* g) {
    if (int st = rs_check_ratio(name, up, down)) return st;
    g->zeros = K >= 1 && K <= SCH_MAX_H ? rs_zeros_of(up, down, K) : 0;
    if (g->zeros) g->plan = sch_plan(up, down, g->zeros, to16k);                          // H sizes the state; params() reports what is wrong
    auto params = [&]() -> int {
        NELE_CHECK_ARG(g->zeros, "%s: K=%d is not the table width of up=%d, down=%d for any zeros in 1 .. %d", name, K, up, down, RS_MAX_ZEROS);
        return sch_check_plan(name, up, down, g->zeros, to16k, &g->plan);
    };
    return slot_state_check(name, state, state_bytes, S, params, nele_sched_stream_state_bytes(S, g->plan.H), "nele_sched_stream_state_bytes",
                            g->plan.H);
}

// slots == null: every record; write_hdr: the header too
int sch_reset(const char* name, void* state, int S, int up, int down, int K, int to16k, const SchPlan& p, const unsigned char* slots, bool write_hdr,
              void* stream) {
    const int hdr[7] = {S, K, up, down, to16k, p.H, p.L0};
    return slot_state_reset(name, state, SCH_HDR_BYTES, sch_rec_bytes(p.H), S, slots, write_hdr ? 7 : 0, hdr, stream, p.L0);
}

}  // namespace

// ============================================================================================ C ABI
extern "C" int nele_sched_stream_plan(int up, int down, int zeros, int to16k, int* info_host) {
    const char* name = "nele_sched_stream_plan";
    NELE_CHECK_ARG(info_host, "%s: null info_host", name);
    SchPlan s;
    if (int st = sch_check_plan(name, up, down, zeros, to16k != 0, &s)) return st;
    info_host[NELE_SCHED_I_K] = s.K;
    info_host[NELE_SCHED_I_D] = s.D;
    info_host[NELE_SCHED_I_L0] = s.L0;
    info_host[NELE_SCHED_I_E] = s.E;
    info_host[NELE_SCHED_I_H] = s.H;
    info_host[NELE_SCHED_I_RNUM] = (int)s.rnum;
    info_host[NELE_SCHED_I_P] = s.P;
    info_host[NELE_SCHED_I_HOP_MIN] = s.hop_min;
    info_host[NELE_SCHED_I_HOP_MAX] = s.hop_max;
    return NELE_OK;
}

extern "C" int nele_sched_stream_widths(int up, int down, int to16k, int pos, int nh, long long* n_in, long long* n_out) {
    const char* name = "nele_sched_stream_widths";
    if (int st = rs_check_ratio(name, up, down)) return st;
    NELE_CHECK_ARG(n_in && n_out, "%s: null n_in or n_out", name);
    const SchPlan s = sch_plan(up, down, 1, to16k != 0);    // the schedule does not depend on zeros
    NELE_CHECK_ARG(pos >= 0 && pos < s.P, "%s: pos=%d outside 0 .. %d, the schedule's period less one", name, pos, s.P - 1);
    NELE_CHECK_ARG(nh >= 1 && nh <= (1 << 20), "%s: nh=%d must be in 1 .. 1048576", name, nh);
    const long long dev = sch_dev_width(s, pos, nh), low = (long long)nh * RS_TILE;
    *n_in = to16k ? dev : low;
    *n_out = to16k ? low : dev;
    return NELE_OK;
}

extern "C" long long nele_sched_stream_record_bytes(int H) {
    if (H < 0 || H > SCH_MAX_H) return -1;
    return sch_rec_bytes(H);
}

extern "C" long long nele_sched_stream_state_bytes(int max_streams, int H) {
    if (max_streams <= 0 || max_streams > SLOT_MAX_STREAMS || H < 0 || H > SCH_MAX_H) return -1;
    return SCH_HDR_BYTES + (long long)max_streams * sch_rec_bytes(H);
}

extern "C" int nele_sched_stream_init(void* state, long long state_bytes, int max_streams, int up, int down, int K, int to16k, void* stream) {
    const char* name = "nele_sched_stream_init";
    SchGeom g{};
    to16k = to16k != 0;
    if (int st = sch_check(name, state, state_bytes, max_streams, up, down, K, to16k, &g)) return st;
    return sch_reset(name, state, max_streams, up, down, K, to16k, g.plan, nullptr, true, stream);
}

extern "C" int nele_sched_stream_reset(void* state, long long state_bytes, int max_streams, int up, int down, int K, int to16k,
                                       const unsigned char* slots, void* stream) {
    const char* name = "nele_sched_stream_reset";
    SchGeom g{};
    to16k = to16k != 0;
    if (int st = sch_check(name, state, state_bytes, max_streams, up, down, K, to16k, &g)) return st;
    return sch_reset(name, state, max_streams, up, down, K, to16k, g.plan, slots, false, stream);
}

extern "C" int nele_sched_stream_hop(void* state, long long state_bytes, int max_streams, int up, int down, int K, int to16k, const double* hp_dev,
                                     const float* x, long long x_stride, const unsigned char* active, int nh, int pos, float* y, long long y_stride,
                                     void* stream) {
    const char* name = "nele_sched_stream_hop";
    SchGeom g{};
    to16k = to16k != 0;
    if (int st = sch_check(name, state, state_bytes, max_streams, up, down, K, to16k, &g)) return st;
    const SchPlan& p = g.plan;
    NELE_CHECK_ARG(hp_dev && x && y, "%s: null table, input or output", name);
    NELE_CHECK_ARG(nh >= 1 && nh <= (1 << 20), "%s: nh=%d must be in 1 .. 1048576", name, nh);
    NELE_CHECK_ARG(pos >= 0 && pos < p.P, "%s: pos=%d outside 0 .. %d, the schedule's period less one", name, pos, p.P - 1);
    const long long dev = sch_dev_width(p, pos, nh), low = (long long)nh * RS_TILE;
    const long long n_in = to16k ? dev : low, n_out = to16k ? low : dev;
    NELE_CHECK_ARG(n_in <= NELE_RESAMPLE_MAX_SAMPLES && n_out <= NELE_RESAMPLE_MAX_SAMPLES, "%s: nh=%d hops are %lld -> %lld samples, more than 2^30 per call",
                   name, nh, n_in, n_out);
    NELE_CHECK_ARG(x_stride >= n_in && y_stride >= n_out, "%s: x_stride=%lld below the call's %lld inputs or y_stride=%lld below its %lld outputs", name,
                   x_stride, n_in, y_stride, n_out);
    SchArgs a{};
    a.state = (unsigned char*)state;
    a.S = max_streams;
    a.up = up;
    a.down = down;
    a.K = K;
    a.H = p.H;
    a.E = p.E;
    a.L0 = p.L0;
    a.to16k = to16k;
    a.span = rs_span(up, down, K);
    a.n_in = (int)n_in;
    a.n_out = (int)n_out;
    a.hp = hp_dev;
    a.x = x;
    a.x_stride = x_stride;
    a.active = active;
    a.y = y;
    a.y_stride = y_stride;
    const bool tab_lds = (long long)up * K * 8 <= RS_TAB_LDS_BYTES;
    const size_t xs = (size_t)(a.span > (p.H + 1) / 2 ? a.span : (p.H + 1) / 2);          // doubles: the span, or the H floats of the new history
    const size_t lds = (xs + (tab_lds ? (size_t)up * K : 0)) * sizeof(double);            // <= 49040 + 16384 bytes: inside the 64 KiB of a plain launch
    const hipStream_t st = as_stream(stream);
    if (tab_lds)
        NELE_PROF("resample_sched", st, hipLaunchKernelGGL(sched_hop_kernel<true>, dim3(max_streams), dim3(RS_TILE), lds, st, a));
    else
        NELE_PROF("resample_sched", st, hipLaunchKernelGGL(sched_hop_kernel<false>, dim3(max_streams), dim3(RS_TILE), lds, st, a));
    NELE_CHECK_LAUNCH(name);
    return NELE_OK;
}
