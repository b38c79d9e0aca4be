// Running ESTOI of the real-time path, many concurrent streams (nele_mon_*): per stream and 256-sample hop, two time-aligned 16 kHz
// signals - r, the clean reference of `lag` hops ago, and y, what the listener hears (deg + add) - go through ESTOI's own chain with
// state instead of the whole utterance.  All arithmetic float64 behind float32 inputs (tests/monitor_ref.py):
//   resampling  16 -> 10 kHz on ESTOI's 581-tap filter (es_filter_tap, csrc/estoi_defs.h): output m is final once input
//               floor((8 m + 290) / 5) has arrived; measured hop t makes outputs 160 t - 36 .. 160 t + 123 from its 256 samples and the
//               128 before them, each the sum over inputs in ascending order that the batch kernel forms
//   frames      256 at hop 128, Hann(258)[1:-1]; energy of r in dB, kept iff finite and above the RUNNING maximum - 40 dB (the batch
//               measure gates on the global maximum); 0, 1 or 2 frames per hop
//   re-analysis kept position i of the overlap-added kept frames needs kept frames i - 1, i, i + 1: it is windowed again and transformed
//               when kept frame i + 1 arrives (r and y share one complex transform, fft512.h's pair packing), 15 third-octave bands
//               (c_tob_lo / c_tob_hi), into a ring of the last 30 band vectors
//   segment     from the 30th band vector on: row then column normalisation of both 15 x 30 blocks, oldest column first, d = the mean
//               product; a finite d is counted, summed and smoothed, any other only counted as skipped
//   mon_table_kernel : the filter by phase, the window and the twiddles, once per state (nele_mon_init), behind the geometry header
//   mon_hop_kernel   : one wave per stream, one stream per workgroup, looping over the call's hops with the record in LDS
// lim_hop_kernel's shape (csrc/limiter.hip): state is read and written with plain loads and stores by the stream's own wave; no atomics,
// no workgroup barrier, nothing crosses waves, and a record passes through memory exactly as it sits in LDS: a slot's bits do not depend
// on the hop grouping, on max_streams or on the other slots.
#include "common.h"
#include "estoi_defs.h"
#include "fft512.h"
#include "slot_state.h"
#include <cmath>
#include "../../include/nele_hip_ext10.h"

namespace {

#define MON_BLK NELE_MON_HOP                               // samples per hop at 16 kHz
#define MON_OUT 160                                        // samples per hop at 10 kHz
#define MON_BEHIND 36                                      // 10 kHz samples of a hop that only the next hop can finish
#define MON_M 117                                          // taps per phase: tap p + 5 m, m = 0 .. 116
#define MON_MPAD 120                                       // a phase's row in the table (zeros behind tap 580)
#define MON_HIST 128                                       // 16 kHz samples carried: output -36 of a hop reads back to sample -115
#define MON_T10 416                                        // 10 kHz samples in flight at most: 255 carried + 160
#define MON_BPAD 16                                        // doubles per place of the ring: 15 bands
constexpr long long MON_O_TAPS = SLOT_GEOM_HDR_BYTES;      // header: int [0] = max_streams, [1] = the record's bytes, [2] = lag, [3] = NELE_MON_STATS
constexpr long long MON_O_WIN = MON_O_TAPS + slot_al(8LL * 5 * MON_MPAD);      // 5120
constexpr long long MON_O_TW = MON_O_WIN + 8LL * ES_NFRAME;                    // 7168
constexpr long long MON_HDR_BYTES = MON_O_TW + 16LL * 256;                     // 11264
// per-stream record, byte offsets
constexpr long long MON_O_CTL = 0;                         // int [8], see MonCtl
constexpr long long MON_O_STATS = 64;                      // double [NELE_MON_STATS]
constexpr long long MON_O_HIST = 256;                      // double [2][128]
constexpr long long MON_O_TAIL = MON_O_HIST + 8LL * 2 * MON_HIST;              // double [2][256]
constexpr long long MON_O_A = MON_O_TAIL + 8LL * 2 * ES_NFRAME;                // double [2][128]
constexpr long long MON_O_HI = MON_O_A + 8LL * 2 * ES_HOP;                     // double [2][128]
constexpr long long MON_O_RING = MON_O_HI + 8LL * 2 * ES_HOP;                  // double [2][30][16]
constexpr long long MON_O_REF = MON_O_RING + 8LL * 2 * ES_NSEG * MON_BPAD;     // float [4][256]
constexpr long long MON_REC_BYTES = MON_O_REF + 4LL * NELE_MON_MAX_LAG * MON_BLK;
static_assert(MON_O_WIN == 5120 && MON_O_TW == 7168 && MON_HDR_BYTES == 11264 && MON_HDR_BYTES % 256 == 0, "the tables of section 27");
static_assert(MON_O_TAIL == 2304 && MON_O_A == 6400 && MON_O_HI == 8448 && MON_O_RING == 10496 && MON_O_REF == 18176 &&
                  MON_REC_BYTES == 22272 && MON_REC_BYTES % 256 == 0,
              "the record of section 27");
// output j = -36 .. 123 of a hop: its newest input is sample floor((8 j + 290) / 5) of the hop, its oldest 116 before that
static_assert((8 * (MON_OUT - MON_BEHIND - 1) + ES_HALF) / 5 < MON_BLK && (8 * -MON_BEHIND + ES_HALF) / 5 - (MON_M - 1) >= -MON_HIST &&
                  8 * -MON_BEHIND + ES_HALF >= 0 && 5 * MON_BLK == 8 * MON_OUT && 5 * (MON_M - 1) <= 2 * ES_HALF && 5 * MON_MPAD > 2 * ES_HALF + 4,
              "the resampler's reach");
static_assert(ES_NFRAME - 1 + MON_OUT < MON_T10, "the 10 kHz samples in flight");

enum MonCtl { C_NIN = 0, C_HPOS, C_STARTED, C_NTAIL, C_KC, C_NVEC, C_RPOS, C_HASM };
enum MonStat { S_COUNT = 0, S_SUM, S_LAST, S_SMOOTH, S_SKIPPED, S_SEEN, S_KEPT, S_M };

struct MonArgs {
    unsigned char* state;
    int S;
    const float* ref;            // [S][ld]
    const float* deg;            // [S][ld] or null (the delayed ref)
    const float* add;            // [S][ld] or null
    long long ld;
    const unsigned char* active; // [S] or null (all)
    int nh;
    double alpha;
    double* stats;               // [S][NELE_MON_STATS] or null
    double* seg;                 // [S][nh][2] or null
    int* nseg;                   // [S][nh] or null
};

// grid 1, block 1024: the tables behind the geometry header
__global__ void mon_table_kernel(unsigned char* __restrict__ state) {
    __shared__ double red[16];
    const int t = threadIdx.x;
    const double v = es_filter_tap(t, red);                // 0 for t > 580
    double* hp = reinterpret_cast<double*>(state + MON_O_TAPS);
    if (t < 5 * MON_MPAD) hp[(t % 5) * MON_MPAD + t / 5] = v;
    if (t < ES_NFRAME) {
        reinterpret_cast<double*>(state + MON_O_WIN)[t] = hann_sym256(t);
        reinterpret_cast<double2*>(state + MON_O_TW)[t] = fft512_twiddle(t);
    }
}

__global__ __launch_bounds__(64) void mon_hop_kernel(MonArgs a) {
    __shared__ double hp[5 * MON_MPAD];                    // tap p + 5 m at [p * 120 + m]
    __shared__ double hw[ES_NFRAME];
    __shared__ double2 tw[256];
    __shared__ double xin[2][MON_HIST + MON_BLK];          // r, y at 16 kHz: sample n of the hop at [128 + n]
    __shared__ double t10[2][MON_T10];                     // r, y at 10 kHz, from the first sample no frame has left behind
    __shared__ double fr[2][ES_NFRAME];                    // the windowed frame
    __shared__ double ov[2][ES_NFRAME];                    // [0 .. 127] the next re-analysis frame's first half, [128 .. 255] the last kept frame's second
    __shared__ double rg[2][ES_NSEG][MON_BPAD];
    __shared__ __attribute__((aligned(16))) double2 xw[FFTW_SLOTS];   // the transform's exchange buffer; the band powers and the segment's blocks overlay it
    __shared__ double part[ES_NSEG];
    const int lane = threadIdx.x, b = blockIdx.x;
    if (b >= a.S) return;
    if (a.active && !a.active[b]) return;                  // neither read nor written
    const int lag = reinterpret_cast<const int*>(a.state)[2];
    if (lag < 0 || lag > NELE_MON_MAX_LAG || !slot_hdr_matches(a.state, a.S, (int)MON_REC_BYTES, lag, NELE_MON_STATS)) return;   // not nele_mon_init's: touch nothing
    {
        const double* g = reinterpret_cast<const double*>(a.state + MON_O_TAPS);
        for (int i = lane; i < 5 * MON_MPAD; i += 64) hp[i] = g[i];
        const double* gw = reinterpret_cast<const double*>(a.state + MON_O_WIN);
        const double2* gt = reinterpret_cast<const double2*>(a.state + MON_O_TW);
        for (int i = lane; i < ES_NFRAME; i += 64) {
            hw[i] = gw[i];
            tw[i] = gt[i];
        }
    }
    unsigned char* rec = a.state + MON_HDR_BYTES + (size_t)b * MON_REC_BYTES;
    int* ctlp = reinterpret_cast<int*>(rec + MON_O_CTL);
    double* statp = reinterpret_cast<double*>(rec + MON_O_STATS);
    double* histp = reinterpret_cast<double*>(rec + MON_O_HIST);
    double* tailp = reinterpret_cast<double*>(rec + MON_O_TAIL);
    double* ap = reinterpret_cast<double*>(rec + MON_O_A);
    double* hip = reinterpret_cast<double*>(rec + MON_O_HI);
    double* ringp = reinterpret_cast<double*>(rec + MON_O_RING);
    float* refp = reinterpret_cast<float*>(rec + MON_O_REF);

    // every lane holds the counters and the readings: the wave's control flow is uniform
    int nin = ctlp[C_NIN], hpos = ctlp[C_HPOS], started = ctlp[C_STARTED], ntail = ctlp[C_NTAIL], kc = ctlp[C_KC], nvec = ctlp[C_NVEC],
        rpos = ctlp[C_RPOS], hasM = ctlp[C_HASM];
    hpos = (lag > 0 && hpos >= 0 && hpos < lag) ? hpos : 0;                    // (a record only nele_mon_init / _reset and this kernel write
    ntail = min(max(ntail, 0), ES_NFRAME - 1);                                 //  holds these ranges; an index never leaves the arrays)
    rpos = min(max(rpos, 0), ES_NSEG - 1);
    double st[NELE_MON_STATS];
#pragma unroll
    for (int i = 0; i < NELE_MON_STATS; ++i) st[i] = statp[i];
    for (int i = lane; i < 2 * MON_HIST; i += 64) xin[i / MON_HIST][i % MON_HIST] = histp[i];
    for (int i = lane; i < 2 * ES_NFRAME; i += 64) t10[i / ES_NFRAME][i % ES_NFRAME] = tailp[i];
    for (int i = lane; i < 2 * ES_HOP; i += 64) {
        ov[i / ES_HOP][i % ES_HOP] = ap[i];
        ov[i / ES_HOP][ES_HOP + i % ES_HOP] = hip[i];
    }
    for (int i = lane; i < 2 * ES_NSEG * MON_BPAD; i += 64) (&rg[0][0][0])[i] = ringp[i];
    fftw_wave_sync();

    const float* refb = a.ref + (size_t)b * a.ld;
    const float* degb = a.deg ? a.deg + (size_t)b * a.ld : nullptr;
    const float* addb = a.add ? a.add + (size_t)b * a.ld : nullptr;
    double* p2x = reinterpret_cast<double*>(xw);           // |X|^2, |Y|^2 of bins 0 .. 255
    double* p2y = p2x + 256;
    double* sx = reinterpret_cast<double*>(xw);            // the segment's blocks [15][31]
    double* sy = sx + ES_NB * (ES_NSEG + 1);
    static_assert(2 * ES_NB * (ES_NSEG + 1) <= 2 * FFTW_SLOTS, "the segment's blocks fit the exchange buffer");
    const double nan = __longlong_as_double(0x7ff8000000000000LL);

    for (int h = 0; h < a.nh; ++h) {
        const size_t col = (size_t)h * MON_BLK;
        float rv[4], dg[4] = {0.f, 0.f, 0.f, 0.f}, ad[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) rv[i] = refb[col + 64 * i + lane];
        if (degb) {
#pragma unroll
            for (int i = 0; i < 4; ++i) dg[i] = degb[col + 64 * i + lane];
        }
        if (addb) {
#pragma unroll
            for (int i = 0; i < 4; ++i) ad[i] = addb[col + 64 * i + lane];
        }
        if (lag > 0) {                                     // the hop of `lag` hops ago leaves the history, this one enters; each lane its own four places
            float* hh = refp + hpos * MON_BLK;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float old = hh[64 * i + lane];
                hh[64 * i + lane] = rv[i];
                rv[i] = old;
            }
            hpos = (hpos + 1 == lag) ? 0 : hpos + 1;
        }
        int ns = 0;
        double sd0 = nan, sd1 = nan;
        if (nin < lag) {
            ++nin;                                         // nothing to compare with yet
        } else {
            // ---- 1. r and y of this hop, float64
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                double y = degb ? (double)dg[i] : (double)rv[i];
                if (addb) y += (double)ad[i];
                xin[0][MON_HIST + 64 * i + lane] = (double)rv[i];
                xin[1][MON_HIST + 64 * i + lane] = y;
            }
            fftw_wave_sync();
            // ---- 2. the hop's 160 outputs at 10 kHz (the stream's first hop: 124, outputs 0 .. 123), five per lane
            const int skip = started ? 0 : MON_BEHIND;
#pragma unroll
            for (int q = 0; q < 2 * MON_OUT / 64; ++q) {
                const int e = lane + 64 * q, sig = e / MON_OUT, jj = e - sig * MON_OUT;
                const int c = 8 * (jj - MON_BEHIND) + ES_HALF, top = c / 5;
                const double* xs = &xin[sig][MON_HIST + top];
                const int p = c - 5 * top;
                const double* hh = &hp[p * MON_MPAD];
                double acc = 0.0;                           // taps p + 5 m <= 580 only: a sample that is not a number reaches no output it has no tap in
                for (int m = p ? MON_M - 2 : MON_M - 1; m >= 0; --m) acc += xs[-m] * hh[m];    // inputs in ascending order
                if (jj >= skip) t10[sig][ntail + jj - skip] = acc;
            }
            ntail += MON_OUT - skip;
            started = 1;
            double keepx[4];                               // the last 128 samples become the history
#pragma unroll
            for (int i = 0; i < 4; ++i) keepx[i] = xin[i >> 1][MON_BLK + 64 * (i & 1) + lane];
            fftw_wave_sync();
#pragma unroll
            for (int i = 0; i < 4; ++i) xin[i >> 1][64 * (i & 1) + lane] = keepx[i];
            // ---- 3. the frames these samples complete
            int foff = 0;
            while (ntail - foff >= ES_NFRAME) {
                double ex = 0.0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int j = lane + 64 * i;
                    const double wx = hw[j] * t10[0][foff + j], wy = hw[j] * t10[1][foff + j];
                    fr[0][j] = wx;
                    fr[1][j] = wy;
                    ex += wx * wx;
                }
                ex = wave_sum(ex);
                const double en = 20.0 * log10(sqrt(ex) + ES_EPS);
                foff += ES_HOP;
                st[S_SEEN] += 1.0;
                const bool fin = isfinite(en);
                if (fin) {
                    st[S_M] = hasM ? fmax(st[S_M], en) : en;
                    hasM = 1;
                }
                fftw_wave_sync();
                if (!(fin && (st[S_M] - 40.0 - en) < 0.0)) continue;           // silent, or not a number: dropped
                st[S_KEPT] += 1.0;
                if (kc == 0) {                             // the first kept frame: zeros before it
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        ov[0][lane + 64 * i] = fr[0][lane + 64 * i];
                        ov[1][lane + 64 * i] = fr[1][lane + 64 * i];
                    }
                    kc = 1;
                    fftw_wave_sync();
                    continue;
                }
                kc = 2;
                // ---- 4. the re-analysis frame of the kept frame before this one: [first half carried | its second half + this one's first]
                double2 v[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const int j = fftw_n(lane, r);
                    double xs_ = 0.0, ys_ = 0.0;
                    if (j < ES_NFRAME) {
                        xs_ = ov[0][j];
                        ys_ = ov[1][j];
                        if (j >= ES_HOP) {
                            xs_ += fr[0][j - ES_HOP];
                            ys_ += fr[1][j - ES_HOP];
                        }
                        xs_ *= hw[j];
                        ys_ *= hw[j];
                    }
                    v[r] = make_double2(xs_, ys_);
                }
                double na[4], nhi[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int sig = i >> 1, j = 64 * (i & 1) + lane;
                    na[i] = ov[sig][ES_HOP + j] + fr[sig][j];
                    nhi[i] = fr[sig][ES_HOP + j];
                }
                fftw_wave_sync();
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int sig = i >> 1, j = 64 * (i & 1) + lane;
                    ov[sig][j] = na[i];
                    ov[sig][ES_HOP + j] = nhi[i];
                }
                fft512_wave<false>(v, xw, tw, lane);
                fft512_wave_store(v, xw, lane);
                double px[4], py[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int q = lane + 64 * i;            // bins 0 .. 255; the bands end at 218
                    const double2 zk = xw[fftw_slot(q)], zn = xw[fftw_slot((512 - q) & 511)];
                    double2 A, Bv;
                    fft512_pair_split(zk, zn, A, Bv);
                    px[i] = A.x * A.x + A.y * A.y;
                    py[i] = Bv.x * Bv.x + Bv.y * Bv.y;
                }
                fftw_wave_sync();
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    p2x[lane + 64 * i] = px[i];
                    p2y[lane + 64 * i] = py[i];
                }
                fftw_wave_sync();
                if (lane < 2 * ES_NB) {
                    const int sig = lane / ES_NB, band = lane - sig * ES_NB;
                    const double* pp = sig ? p2y : p2x;
                    double s = 0.0;
                    for (int q = c_tob_lo[band]; q < c_tob_hi[band]; ++q) s += pp[q];
                    rg[sig][rpos][band] = sqrt(s);
                }
                rpos = (rpos + 1 == ES_NSEG) ? 0 : rpos + 1;                   // now the oldest place
                nvec = min(nvec + 1, ES_NSEG);
                fftw_wave_sync();
                if (nvec < ES_NSEG) continue;
                // ---- 5. the segment of the last 30 band vectors, oldest column first (estoi_seg_kernel's arithmetic)
                for (int i = lane; i < ES_NB * ES_NSEG; i += 64) {
                    const int r = i / ES_NSEG, c = i - r * ES_NSEG;
                    int place = rpos + c;
                    place -= place >= ES_NSEG ? ES_NSEG : 0;
                    sx[r * (ES_NSEG + 1) + c] = rg[0][place][r];
                    sy[r * (ES_NSEG + 1) + c] = rg[1][place][r];
                }
                fftw_wave_sync();
                if (lane < 2 * ES_NB) {                    // rows: subtract the mean over time, divide by the norm
                    double* q = ((lane < ES_NB) ? sx : sy) + (lane % ES_NB) * (ES_NSEG + 1);
                    double mu = 0.0;
                    for (int c = 0; c < ES_NSEG; ++c) mu += q[c];
                    mu /= (double)ES_NSEG;
                    double nn = 0.0;
                    for (int c = 0; c < ES_NSEG; ++c) {
                        const double u = q[c] - mu;
                        q[c] = u;
                        nn += u * u;
                    }
                    const double inv = 1.0 / sqrt(nn);
                    for (int c = 0; c < ES_NSEG; ++c) q[c] *= inv;
                }
                fftw_wave_sync();
                if (lane < 2 * ES_NSEG) {                  // columns: subtract the mean over bands, divide by the norm
                    double* q = ((lane < ES_NSEG) ? sx : sy) + lane % ES_NSEG;
                    double mu = 0.0;
                    for (int r = 0; r < ES_NB; ++r) mu += q[r * (ES_NSEG + 1)];
                    mu /= (double)ES_NB;
                    double nn = 0.0;
                    for (int r = 0; r < ES_NB; ++r) {
                        const double u = q[r * (ES_NSEG + 1)] - mu;
                        q[r * (ES_NSEG + 1)] = u;
                        nn += u * u;
                    }
                    const double inv = 1.0 / sqrt(nn);
                    for (int r = 0; r < ES_NB; ++r) q[r * (ES_NSEG + 1)] *= inv;
                }
                fftw_wave_sync();
                if (lane < ES_NSEG) {
                    double s = 0.0;
                    for (int r = 0; r < ES_NB; ++r) s += sx[r * (ES_NSEG + 1) + lane] * sy[r * (ES_NSEG + 1) + lane];
                    part[lane] = s;
                }
                fftw_wave_sync();
                double d = 0.0;
                for (int c = 0; c < ES_NSEG; ++c) d += part[c];
                d /= (double)ES_NSEG;
                fftw_wave_sync();                          // part and the blocks are read: the next frame may restage them
                const bool ok = isfinite(d);
                if (ns == 0) sd0 = ok ? d : nan;
                else sd1 = ok ? d : nan;
                ++ns;
                if (ok) {
                    st[S_SMOOTH] = (st[S_COUNT] == 0.0) ? d : st[S_SMOOTH] + a.alpha * (d - st[S_SMOOTH]);
                    st[S_COUNT] += 1.0;
                    st[S_SUM] += d;
                    st[S_LAST] = d;
                } else {
                    st[S_SKIPPED] += 1.0;
                }
            }
            // ---- 6. the samples no frame has left behind move to the front
            if (foff > 0) {
                const int n = ntail - foff;                // < 256
                double mv[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int j = 64 * (i & 3) + lane;
                    mv[i] = j < n ? t10[i >> 2][foff + j] : 0.0;
                }
                fftw_wave_sync();
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int j = 64 * (i & 3) + lane;
                    if (j < n) t10[i >> 2][j] = mv[i];
                }
                ntail = n;
                fftw_wave_sync();
            }
        }
        if (a.nseg && lane == 0) a.nseg[(size_t)b * a.nh + h] = ns;
        if (a.seg && lane < 2) a.seg[((size_t)b * a.nh + h) * 2 + lane] = lane ? sd1 : sd0;
    }

    // ---- the record goes back as it sits in LDS (zeros behind the carried 10 kHz samples)
    fftw_wave_sync();
    for (int i = lane; i < 2 * MON_HIST; i += 64) histp[i] = xin[i / MON_HIST][i % MON_HIST];
    for (int i = lane; i < 2 * ES_NFRAME; i += 64) tailp[i] = (i % ES_NFRAME) < ntail ? t10[i / ES_NFRAME][i % ES_NFRAME] : 0.0;
    for (int i = lane; i < 2 * ES_HOP; i += 64) {
        ap[i] = ov[i / ES_HOP][i % ES_HOP];
        hip[i] = ov[i / ES_HOP][ES_HOP + i % ES_HOP];
    }
    for (int i = lane; i < 2 * ES_NSEG * MON_BPAD; i += 64) ringp[i] = (&rg[0][0][0])[i];
    if (lane == 0) {
        ctlp[C_NIN] = nin; ctlp[C_HPOS] = hpos; ctlp[C_STARTED] = started; ctlp[C_NTAIL] = ntail;
        ctlp[C_KC] = kc; ctlp[C_NVEC] = nvec; ctlp[C_RPOS] = rpos; ctlp[C_HASM] = hasM;
#pragma unroll
        for (int i = 0; i < NELE_MON_STATS; ++i) statp[i] = st[i];
        if (a.stats) {
#pragma unroll
            for (int i = 0; i < NELE_MON_STATS; ++i)
                a.stats[(size_t)b * NELE_MON_STATS + i] = (i == S_M && !hasM) ? -HUGE_VAL : st[i];
        }
    }
}

int mon_check(const char* name, const void* state, long long state_bytes, int S) {
    return slot_state_check(name, state, state_bytes, S, []() -> int { return NELE_OK; }, nele_mon_state_bytes(S), "nele_mon_state_bytes");
}

}  // namespace

// ============================================================================================ C ABI
extern "C" long long nele_mon_stream_record_bytes(void) { return MON_REC_BYTES; }

extern "C" long long nele_mon_state_bytes(int max_streams) {
    if (max_streams <= 0 || max_streams > SLOT_MAX_STREAMS) return -1;
    return MON_HDR_BYTES + (long long)max_streams * MON_REC_BYTES;
}

extern "C" int nele_mon_init(void* state, long long state_bytes, int max_streams, int lag, void* stream) {
    const char* name = "nele_mon_init";
    NELE_CHECK_ARG(lag >= 0 && lag <= NELE_MON_MAX_LAG, "%s: lag=%d must be in 0 .. %d hops", name, lag, NELE_MON_MAX_LAG);
    int st = mon_check(name, state, state_bytes, max_streams);
    if (st) return st;
    const int hdr[4] = {max_streams, (int)MON_REC_BYTES, lag, NELE_MON_STATS};
    st = slot_state_reset(name, state, MON_HDR_BYTES, MON_REC_BYTES, max_streams, nullptr, 4, hdr, stream);
    if (st) return st;
    hipLaunchKernelGGL(mon_table_kernel, dim3(1), dim3(1024), 0, as_stream(stream), (unsigned char*)state);
    NELE_CHECK_LAUNCH(name);
    return NELE_OK;
}

extern "C" int nele_mon_reset(void* state, long long state_bytes, int max_streams, const unsigned char* slots, void* stream) {
    const char* name = "nele_mon_reset";
    int st = mon_check(name, state, state_bytes, max_streams);
    if (st) return st;
    return slot_state_reset(name, state, MON_HDR_BYTES, MON_REC_BYTES, max_streams, slots, 0, nullptr, stream);
}

extern "C" int nele_mon_hop(void* state, long long state_bytes, int max_streams, const float* ref, const float* deg, const float* add,
                            const unsigned char* active, int nh, double alpha, double* stats, double* seg, int* nseg, void* stream) {
    const char* name = "nele_mon_hop";
    int st = mon_check(name, state, state_bytes, max_streams);
    if (st) return st;
    NELE_CHECK_ARG(ref, "%s: null ref", name);
    NELE_CHECK_ARG(nh >= 1 && nh <= (1 << 20), "%s: nh=%d must be in 1 .. 1048576", name, nh);
    NELE_CHECK_ARG(alpha > 0.0 && alpha <= 1.0, "%s: alpha=%g must be in (0, 1]", name, alpha);
    MonArgs a{};
    a.state = (unsigned char*)state;
    a.S = max_streams;
    a.ref = ref;
    a.deg = deg;
    a.add = add;
    a.ld = (long long)nh * MON_BLK;
    a.active = active;
    a.nh = nh;
    a.alpha = alpha;
    a.stats = stats;
    a.seg = seg;
    a.nseg = nseg;
    hipLaunchKernelGGL(mon_hop_kernel, dim3(max_streams), dim3(64), 0, as_stream(stream), a);
    NELE_CHECK_LAUNCH(name);
    return NELE_OK;
}
