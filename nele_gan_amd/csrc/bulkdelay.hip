// Bulk-delay search and alignment ahead of the echo canceller (nele_bulk_*, include/nele_hip_ext.h): per stream slot, the whole number
// of hops by which `played` reaches the microphone late, found from SCOT-weighted cross-spectra against the last Q far-end blocks, and
// a delay line that hands `played` on late by it.  256-sample hops, 512-point float64 transforms (fft512.h), the packed spectra of
// csrc/aec.hip (256 double2: slot k = bin k, slot 0 = (bin 0, bin 256), products component-wise in slot 0).  The arithmetic is DESIGN.md
// section 16; tests/bulk_ref.py restates it in numpy.
//   bulk_hop_kernel    : one workgroup per stream and call, looping over the call's hops
//   bulk_set_kernel    : nele_bulk_set_delay, one thread per slot
//   bulk_status_kernel : nele_bulk_status, one workgroup per slot
// While a slot searches, each hop runs the search step of csrc/bulk_search.h (shared with csrc/bulktrack.hip): every operand is the
// stream's own, every sum has a fixed order: a slot's bits do not depend on the hop grouping, on B or on the other slots.  Once locked,
// a workgroup-uniform branch leaves only the delay line.  State is read and written with plain loads and stores by the stream's own
// workgroup; no atomics, nothing crosses workgroups.
#include "common.h"
#include "fft512.h"
#include "slot_state.h"
#include "bulk_search.h"
#include "../../include/nele_hip_ext.h"

namespace {

constexpr long long BULK_HDR_BYTES = SLOT_GEOM_HDR_BYTES;  // int [0] = max_streams, [1] = blocks (what nele_bulk_init was given)
// per-stream record, byte offsets.  A cleared record is a fresh slot, so cand and delay are kept plus one (0 = none / searching).
constexpr long long BULK_O_META = 0;                       // int [8]: BULK_M_*
constexpr long long BULK_O_CONF = 32;                      // double: conf of the last evaluated hop
constexpr long long BULK_O_E = 256;                        // double [64]: e_q of the last evaluated hop
constexpr long long BULK_O_XPREV = BULK_O_E + 8 * BULK_MAXQ;        // float [256]: the previous hop of `played` while searching
constexpr long long BULK_O_SD = BULK_O_XPREV + 4 * BULK_BLK;        // double [257 (+ 7)]: S_d
constexpr long long BULK_O_SX = BULK_O_SD + 8 * 264;                // double [257 (+ 7)]: S_x
constexpr long long BULK_O_LINE = slot_al(BULK_O_SX + 8 * 264);     // float [Q][256]: the delay line, hop of k hops ago at (lhead - k) mod Q
__host__ __device__ constexpr long long bulk_o_x(int Q) { return BULK_O_LINE + 4LL * BULK_BLK * Q; }    // double2 [Q][256]: X_q at (head + q) % Q
__host__ __device__ constexpr long long bulk_o_c(int Q) { return bulk_o_x(Q) + 16LL * BULK_BLK * Q; }   // double2 [Q][256]: C_q
__host__ __device__ constexpr long long bulk_rec_bytes(int Q) { return slot_al(bulk_o_c(Q) + 16LL * BULK_BLK * Q); }
enum { BULK_M_HEAD = 0, BULK_M_LHEAD = 1, BULK_M_N = 2, BULK_M_CAND1 = 3, BULK_M_RUN = 4, BULK_M_DELAY1 = 5 };

struct BulkArgs {
    unsigned char* state;
    int S, Q;
    const float* mic;            // [S][ld]
    const float* played;
    long long ld;
    const unsigned char* active; // [S] or null (all)
    int nh;
    double lambda, ratio;
    int hold;
    float* aligned;              // [S][ld]
    int* delay_hops;             // [S] or null
};

__global__ __launch_bounds__(256) void bulk_hop_kernel(BulkArgs a) {
    __shared__ BulkSearchLds lds;
    __shared__ int s_delay;
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= a.S) return;
    if (a.active && !a.active[b]) return;                  // neither read nor written
    if (!slot_hdr_matches(a.state, a.S, a.Q)) return;      // not the state nele_bulk_init laid out for (S, Q): touch nothing
    const int Q = a.Q;
    unsigned char* rec = a.state + BULK_HDR_BYTES + (size_t)b * bulk_rec_bytes(Q);
    int* meta = reinterpret_cast<int*>(rec + BULK_O_META);
    float* line = reinterpret_cast<float*>(rec + BULK_O_LINE);
    BulkSearchRec R;
    R.confp = reinterpret_cast<double*>(rec + BULK_O_CONF);
    R.erec = reinterpret_cast<double*>(rec + BULK_O_E);
    R.xprev = reinterpret_cast<float*>(rec + BULK_O_XPREV);
    R.Sdp = reinterpret_cast<double*>(rec + BULK_O_SD);
    R.Sxp = reinterpret_cast<double*>(rec + BULK_O_SX);
    R.ring = reinterpret_cast<double2*>(rec + bulk_o_x(Q));
    R.Cst = reinterpret_cast<double2*>(rec + bulk_o_c(Q));
    const bool slot0 = (t == 0);

    BulkSearchRegs g;
    g.head = min(max(meta[BULK_M_HEAD], 0), Q - 1);
    int lhead = min(max(meta[BULK_M_LHEAD], 0), Q - 1);
    g.n = meta[BULK_M_N];
    g.cand = meta[BULK_M_CAND1] - 1;
    g.run = meta[BULK_M_RUN];
    int delay = min(meta[BULK_M_DELAY1], Q) - 1;           // workgroup-uniform throughout
    const bool searched = delay < 0;                       // the search state is read, and written back, only by a slot that came in searching
    g.sd = g.sx = g.sd_ny = g.sx_ny = 0.0;
    if (searched) bulk_search_load(lds, R, g, t);
    const float* micb = a.mic + (size_t)b * a.ld;
    const float* plb = a.played + (size_t)b * a.ld;
    float* outb = a.aligned + (size_t)b * a.ld;
    __syncthreads();

    for (int h = 0; h < a.nh; ++h) {
        const size_t col = (size_t)h * BULK_BLK;
        // ---- 1. push x onto the delay line (thread t: sample t of every hop, so its own earlier stores are what it reads back)
        const float xv = plb[col + t];
        lhead = (lhead + 1 == Q) ? 0 : lhead + 1;
        line[(size_t)lhead * BULK_BLK + t] = xv;
        if (delay < 0) {
            // ---- 2. the search step; the lock is a run of `hold` hops (thread 0 decides)
            int qs = 0;
            if (bulk_search_step(lds, R, g, Q, xv, micb[col + t], a.lambda, a.ratio, t, qs)) {
                if (slot0) s_delay = (g.run >= a.hold) ? max(qs - 1, 0) : -1;
                __syncthreads();
                delay = s_delay;
            }
        }
        // ---- 3. the output hop: zeros while searching, then the delay line's entry of `delay` hops ago
        float y = 0.0f;
        if (delay == 0) {
            y = xv;
        } else if (delay > 0) {
            int lp = lhead - delay;
            if (lp < 0) lp += Q;
            y = line[(size_t)lp * BULK_BLK + t];
        }
        outb[col + t] = y;
    }
    if (searched) bulk_search_store(lds, R, g, t);
    if (slot0) {
        meta[BULK_M_LHEAD] = lhead;
        if (searched) {
            meta[BULK_M_HEAD] = g.head;
            meta[BULK_M_N] = g.n;
            meta[BULK_M_CAND1] = g.cand + 1;
            meta[BULK_M_RUN] = g.run;
            meta[BULK_M_DELAY1] = delay + 1;
        }
        if (a.delay_hops) a.delay_hops[b] = delay;
    }
}

__global__ __launch_bounds__(256) void bulk_set_kernel(unsigned char* state, int S, int Q, const unsigned char* __restrict__ slots,
                                                        const int* __restrict__ delay_hops) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= S || !slot_hdr_matches(state, S, Q)) return;
    if (slots && !slots[b]) return;
    const int d = delay_hops[b];
    if (d < 0 || d >= Q) return;                           // out of range: the slot stays as it is
    int* meta = reinterpret_cast<int*>(state + BULK_HDR_BYTES + (size_t)b * bulk_rec_bytes(Q) + BULK_O_META);
    meta[BULK_M_DELAY1] = d + 1;
}

// grid S, block 64
__global__ __launch_bounds__(64) void bulk_status_kernel(const unsigned char* __restrict__ state, int S, int Q, int* __restrict__ delay_hops,
                                                         int* __restrict__ hops_searched, double* __restrict__ energies,
                                                         double* __restrict__ conf) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= S || !slot_hdr_matches(state, S, Q)) return;
    const unsigned char* rec = state + BULK_HDR_BYTES + (size_t)b * bulk_rec_bytes(Q);
    const int* meta = reinterpret_cast<const int*>(rec + BULK_O_META);
    if (t == 0) {
        if (delay_hops) delay_hops[b] = min(meta[BULK_M_DELAY1], Q) - 1;
        if (hops_searched) hops_searched[b] = meta[BULK_M_N];
        if (conf) conf[b] = *reinterpret_cast<const double*>(rec + BULK_O_CONF);
    }
    if (energies && t < Q) energies[(size_t)b * Q + t] = reinterpret_cast<const double*>(rec + BULK_O_E)[t];
}

int bulk_check(const char* name, const void* state, long long state_bytes, int S, int Q) {
    auto params = [&]() -> int {
        NELE_CHECK_ARG(Q >= 2 && Q <= BULK_MAXQ, "%s: blocks=%d must be in 2 .. %d", name, Q, BULK_MAXQ);
        return NELE_OK;
    };
    return slot_state_check(name, state, state_bytes, S, params, nele_bulk_state_bytes(S, Q), "nele_bulk_state_bytes", Q);
}

// slots == null: every record; write_hdr: the header too
int bulk_reset(const char* name, void* state, int S, int Q, const unsigned char* slots, bool write_hdr, void* stream) {
    const int hdr[2] = {S, Q};
    return slot_state_reset(name, state, BULK_HDR_BYTES, bulk_rec_bytes(Q), S, slots, write_hdr ? 2 : 0, hdr, stream);
}

}  // namespace

// ============================================================================================ C ABI
extern "C" long long nele_bulk_state_bytes(int max_streams, int blocks) {
    if (max_streams <= 0 || max_streams > SLOT_MAX_STREAMS || blocks < 2 || blocks > BULK_MAXQ) return -1;
    return BULK_HDR_BYTES + (long long)max_streams * bulk_rec_bytes(blocks);
}

extern "C" long long nele_bulk_stream_record_bytes(int blocks) {
    if (blocks < 2 || blocks > BULK_MAXQ) return -1;
    return bulk_rec_bytes(blocks);
}

extern "C" int nele_bulk_init(void* state, long long state_bytes, int max_streams, int blocks, void* stream) {
    int st = bulk_check("nele_bulk_init", state, state_bytes, max_streams, blocks);
    if (st) return st;
    return bulk_reset("nele_bulk_init", state, max_streams, blocks, nullptr, true, stream);
}

extern "C" int nele_bulk_reset(void* state, long long state_bytes, int max_streams, int blocks, const unsigned char* slots, void* stream) {
    int st = bulk_check("nele_bulk_reset", state, state_bytes, max_streams, blocks);
    if (st) return st;
    return bulk_reset("nele_bulk_reset", state, max_streams, blocks, slots, false, stream);
}

extern "C" int nele_bulk_set_delay(void* state, long long state_bytes, int max_streams, int blocks, const unsigned char* slots,
                                   const int* delay_hops, void* stream) {
    int st = bulk_check("nele_bulk_set_delay", state, state_bytes, max_streams, blocks);
    if (st) return st;
    NELE_CHECK_ARG(delay_hops, "nele_bulk_set_delay: null delay_hops");
    hipLaunchKernelGGL(bulk_set_kernel, dim3((max_streams + 255) / 256), dim3(256), 0, as_stream(stream), (unsigned char*)state, max_streams, blocks,
                       slots, delay_hops);
    NELE_CHECK_LAUNCH("nele_bulk_set_delay");
    return NELE_OK;
}

extern "C" int nele_bulk_hop(void* state, long long state_bytes, int max_streams, int blocks, const float* mic, const float* played,
                             const unsigned char* active, int nh, double lambda, double ratio, int hold, float* aligned, int* delay_hops,
                             void* stream) {
    int st = bulk_check("nele_bulk_hop", state, state_bytes, max_streams, blocks);
    if (st) return st;
    NELE_CHECK_ARG(mic, "nele_bulk_hop: null mic");
    NELE_CHECK_ARG(played, "nele_bulk_hop: null played");
    NELE_CHECK_ARG(aligned, "nele_bulk_hop: null aligned");
    NELE_CHECK_ARG(nh >= 1 && nh <= (1 << 20), "nele_bulk_hop: nh=%d must be in 1 .. 1048576", nh);
    NELE_CHECK_ARG(lambda > 0.0 && lambda < 1.0, "nele_bulk_hop: lambda=%g must be in (0, 1)", lambda);
    NELE_CHECK_ARG(ratio > 1.0 && ratio <= 1e300, "nele_bulk_hop: ratio=%g must be finite and > 1", ratio);
    NELE_CHECK_ARG(hold >= 1, "nele_bulk_hop: hold=%d must be >= 1", hold);
    BulkArgs a{};
    a.state = (unsigned char*)state;
    a.S = max_streams;
    a.Q = blocks;
    a.mic = mic;
    a.played = played;
    a.ld = (long long)nh * BULK_BLK;
    a.active = active;
    a.nh = nh;
    a.lambda = lambda;
    a.ratio = ratio;
    a.hold = hold;
    a.aligned = aligned;
    a.delay_hops = delay_hops;
    hipLaunchKernelGGL(bulk_hop_kernel, dim3(max_streams), dim3(256), 0, as_stream(stream), a);
    NELE_CHECK_LAUNCH("nele_bulk_hop");
    return NELE_OK;
}

extern "C" int nele_bulk_status(const void* state, long long state_bytes, int max_streams, int blocks, int* delay_hops, int* hops_searched,
                                double* energies, double* conf, void* stream) {
    int st = bulk_check("nele_bulk_status", state, state_bytes, max_streams, blocks);
    if (st) return st;
    hipLaunchKernelGGL(bulk_status_kernel, dim3(max_streams), dim3(64), 0, as_stream(stream), (const unsigned char*)state, max_streams, blocks,
                       delay_hops, hops_searched, energies, conf);
    NELE_CHECK_LAUNCH("nele_bulk_status");
    return NELE_OK;
}
