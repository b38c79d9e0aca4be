// The bulk-delay search of DESIGN.md section 16, step 2, as both modes of csrc/bulkdelay.hip's hop kernel (nele_bulk_hop, nele_track_hop)
// run it: one definition, so that a tracker's background search and a first search are the same operations in the same order.
// For one workgroup of 256 threads that owns one stream slot.  While a slot searches: wave 0 takes ONE complex transform for the two
// real ones ([x_prev, x] + i [0, d]); thread t owns slot t of S_d, S_x and D'; then one wave per pair of blocks (q, q + 1) updates C_q,
// C_q+1 (16-byte accesses, 64 consecutive slots per instruction) and, from hop Q on, takes their two r_q from one Hermitian-packed
// inverse transform and reduces the squares; an odd Q leaves the last block a zero partner.  Pairs are (0, 1), (2, 3), ... whatever the
// ring position, every operand is the stream's own, every sum has a fixed order.
#pragma once
#include "common.h"
#include "fft512.h"
#include "../../include/nele_hip_ext.h"

#define BULK_BLK 256                                       // samples per hop = slots per spectrum
#define BULK_MAXQ NELE_BULK_MAX_BLOCKS

struct BulkSearchLds {                                     // the workgroup's LDS
    double2 tw[256];
    double2 xws[4][FFTW_SLOTS];
    double2 specX[BULK_BLK];                               // X_0
    double2 specD[BULK_BLK];                               // D, then D'
    double ebuf[BULK_MAXQ];
    float xbuf[2 * BULK_BLK];                              // [x_prev, x]
    float dbuf[BULK_BLK];
};

struct BulkSearchRec {                                     // where the slot's record keeps the search state
    double* confp;                                         // conf of the last evaluated hop
    double* erec;                                          // [Q]: e_q of the last evaluated hop
    float* xprev;                                          // [256]
    double* Sdp;                                           // [257]
    double* Sxp;                                           // [257]
    double2* ring;                                         // [Q][256]: X_q at (head + q) % Q
    double2* Cst;                                          // [Q][256]: C_q
};

struct BulkSearchRegs {                                    // what the workgroup keeps in registers over a call's hops
    int head, n, cand, run;                                // (cand, run: thread 0's are the ones that count)
    double sd, sx, sd_ny, sx_ny;                           // S_d, S_x of bin t (thread 0: bins 0 and 256)
};

// the record's x_prev, S_d and S_x into LDS and registers (a barrier before the first bulk_search_step)
__device__ __forceinline__ void bulk_search_load(BulkSearchLds& L, const BulkSearchRec& R, BulkSearchRegs& g, int t) {
    fft512_fill_twiddles(L.tw);
    L.xbuf[t] = R.xprev[t];
    g.sd = R.Sdp[t];
    g.sx = R.Sxp[t];
    if (t == 0) {
        g.sd_ny = R.Sdp[BULK_BLK];
        g.sx_ny = R.Sxp[BULK_BLK];
    }
}

__device__ __forceinline__ void bulk_search_store(const BulkSearchLds& L, const BulkSearchRec& R, const BulkSearchRegs& g, int t) {
    R.xprev[t] = L.xbuf[t];
    R.Sdp[t] = g.sd;
    R.Sxp[t] = g.sx;
    if (t == 0) {
        R.Sdp[BULK_BLK] = g.sd_ny;
        R.Sxp[BULK_BLK] = g.sx_ny;
    }
}

// c <- lambda c + G conj(x) for one slot of a packed spectrum (packed: slot 0, whose two components are the real bins 0 and 256 and
// multiply component-wise).  Which products are fused is written out here (no contraction is left to the compiler in this function), so
// that every build and both kernels that include this file give the bits nele_bulk_hop has always given: the product's real part is
// fma(G.x, x.x, G.y x.y) with G.y x.y rounded first - except where `unfused_real` asks for the sum of the two rounded products, which is
// what bins 1 .. 63 of the first block of a pair have had from the first build on - and its imaginary part fma(G.y, x.x, -(G.x x.y)).
__device__ __forceinline__ double2 bulk_cross_update(double2 c, double2 G, double2 x, double lambda, bool packed, bool unfused_real) {
#pragma clang fp contract(off)
    double2 p;
    if (packed) {
        p = make_double2(G.x * x.x, G.y * x.y);
    } else {
        const double yy = G.y * x.y;
        p.x = unfused_real ? G.x * x.x + yy : fma(G.x, x.x, yy);
        p.y = fma(G.y, x.x, -(G.x * x.y));
    }
    return make_double2(fma(lambda, c.x, p.x), fma(lambda, c.y, p.y));
}

// Section 16's step 2 for one hop: thread t brings sample t of `played` (xv) and of the microphone (dv).  -> whether the hop was
// evaluated (n >= Q, workgroup-uniform).  After an evaluated hop R.erec and R.confp are written and thread 0 holds the updated cand and
// run and, in qs, the leading block; the caller's next barrier is what orders thread 0's reads of ebuf before the next hop's writes.
__device__ __forceinline__ bool bulk_search_step(BulkSearchLds& L, const BulkSearchRec& R, BulkSearchRegs& g, int Q, float xv, float dv,
                                                 double lambda, double ratio, int t, int& qs_out) {
    const int w = t >> 6, lane = t & 63;
    const bool slot0 = (t == 0);
    const double one_m_smooth = 1.0 - NELE_BULK_SMOOTH;
    double2* xw = L.xws[w];
    // ---- 2a. X_0 = rfft512([x_prev, x]) and D = rfft512([0 x 256, d]) from one complex transform (wave 0)
    L.xbuf[BULK_BLK + t] = xv;
    L.dbuf[t] = dv;
    __syncthreads();
    if (w == 0) {
        double2 v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int i = fftw_n(lane, r);
            v[r] = make_double2((double)L.xbuf[i], (i >= BULK_BLK) ? (double)L.dbuf[i - BULK_BLK] : 0.0);
        }
        fftw_wave_sync();                                  // the wave's earlier reads of xw precede the transform's writes
        fft512_wave<false>(v, xw, L.tw, lane);
        fft512_wave_store(v, xw, lane);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            double2 X, D;
            fft512_packed_split(xw, 64 * m + lane, X, D);
            L.specX[64 * m + lane] = X;
            L.specD[64 * m + lane] = D;
        }
    }
    __syncthreads();
    // ---- 2b. the ring moves up one place; S_d, S_x and D' = D / sqrt(S_d S_x + eps) (thread t: slot t)
    L.xbuf[t] = xv;                                        // x_prev <- x (wave 0 has read xbuf; the next write of its upper half is behind a barrier)
    g.head = (g.head == 0) ? Q - 1 : g.head - 1;
    {
        const double2 X0 = L.specX[t], D = L.specD[t];
        R.ring[(size_t)g.head * BULK_BLK + t] = X0;
        double2 Dw;
        if (slot0) {
            g.sd = NELE_BULK_SMOOTH * g.sd + one_m_smooth * (D.x * D.x);
            g.sd_ny = NELE_BULK_SMOOTH * g.sd_ny + one_m_smooth * (D.y * D.y);
            g.sx = NELE_BULK_SMOOTH * g.sx + one_m_smooth * (X0.x * X0.x);
            g.sx_ny = NELE_BULK_SMOOTH * g.sx_ny + one_m_smooth * (X0.y * X0.y);
            Dw = make_double2(D.x / sqrt(g.sd * g.sx + NELE_BULK_EPS), D.y / sqrt(g.sd_ny * g.sx_ny + NELE_BULK_EPS));
        } else {
            g.sd = NELE_BULK_SMOOTH * g.sd + one_m_smooth * (D.x * D.x + D.y * D.y);
            g.sx = NELE_BULK_SMOOTH * g.sx + one_m_smooth * (X0.x * X0.x + X0.y * X0.y);
            const double s = sqrt(g.sd * g.sx + NELE_BULK_EPS);
            Dw = make_double2(D.x / s, D.y / s);
        }
        L.specD[t] = Dw;
    }
    if (g.n < 0x7fffffff) g.n += 1;                        // (a slot that never locks: 2^31 hops are more than a year)
    const bool evaluate = g.n >= Q;
    __syncthreads();                                       // D' and the ring's newest spectrum are the pair loop's operands
    // ---- 2c. C_q <- lambda C_q + D' conj(X_q); e_q = sum of squares of irfft512(C_q)[0 .. 256): one wave per pair of blocks
    for (int pr = w; 2 * pr < Q; pr += 4) {
        const int q0 = 2 * pr, q1 = q0 + 1;
        const bool two = q1 < Q;
        int r0 = g.head + q0, r1 = g.head + q1;
        if (r0 >= Q) r0 -= Q;
        if (r1 >= Q) r1 -= Q;
        const double2* Xa = R.ring + (size_t)r0 * BULK_BLK;
        const double2* Xb = R.ring + (size_t)(two ? r1 : r0) * BULK_BLK;
        double2* Ca = R.Cst + (size_t)q0 * BULK_BLK;
        double2* Cb = R.Cst + (size_t)(two ? q1 : q0) * BULK_BLK;
        fftw_wave_sync();                                  // the previous pair's reads of xw precede these writes
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int k = 64 * m + lane;
            const double2 G = L.specD[k], xa = Xa[k], xb = Xb[k];
            double2 ca = bulk_cross_update(Ca[k], G, xa, lambda, k == 0, m == 0);
            double2 cb = bulk_cross_update(Cb[k], G, xb, lambda, k == 0, false);
            Ca[k] = ca;
            if (two) Cb[k] = cb;
            else cb = make_double2(0.0, 0.0);
            if (evaluate) {
                xw[k] = ca;
                xw[BULK_BLK + k] = cb;
            }
        }
        if (!evaluate) continue;                           // (workgroup-uniform) the first Q - 1 hops only fill the sums
        fftw_wave_sync();
        const double2 a0 = xw[0], b0 = xw[BULK_BLK];
        double2 v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int i = fftw_n(lane, r);
            const int k = ((i <= 256) ? i : 512 - i) & 255;
            v[r] = fft512_packed_join(xw[k], xw[BULK_BLK + k], a0, b0, i);
        }
        fftw_wave_sync();
        fft512_wave<true>(v, xw, L.tw, lane);              // v[m] = 512 (r_q0 + i r_q1)[64 m + lane]; m < 4: the lags 0 .. 255
        double ea = 0.0, eb = 0.0;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const double ra = v[m].x * (1.0 / 512.0), rb = v[m].y * (1.0 / 512.0);
            ea += ra * ra;
            eb += rb * rb;
        }
        ea = wave_sum(ea);
        eb = wave_sum(eb);
        if (lane == 0) {
            L.ebuf[q0] = ea;
            if (two) L.ebuf[q1] = eb;
        }
    }
    // ---- 2d. the leading block and its run (thread 0); what a run of `hold` means is the caller's
    if (evaluate) {
        __syncthreads();
        if (t < Q) R.erec[t] = L.ebuf[t];
        if (slot0) {
            int qs = 0;
            double best = L.ebuf[0];
            for (int q = 1; q < Q; ++q)
                if (L.ebuf[q] > best) {
                    best = L.ebuf[q];
                    qs = q;
                }
            double rest = 0.0;
            for (int q = 0; q < Q; ++q)
                if (q != qs) rest += L.ebuf[q];
            const double lead = best * (double)(Q - 1);
            const bool ok = best > 0.0 && lead >= ratio * rest;
            *R.confp = lead / rest;
            if (ok && qs == g.cand) {
                g.run += 1;
            } else if (ok) {
                g.cand = qs;
                g.run = 1;
            } else {
                g.cand = -1;
                g.run = 0;
            }
            qs_out = qs;
        }
    }
    // (not evaluated: the pair loop's reads of specD and the ring precede their next writes behind the next hop's first barrier)
    return evaluate;
}
