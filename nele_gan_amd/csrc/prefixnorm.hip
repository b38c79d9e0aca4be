// Causal (prefix) energy normalisation of the offline and training paths: the form the real-time path emits (contract
// item 4; rt_head_kernel in realtime.hip), in place of the utterance-level sums of train_nele.py:133-140 / inference.py:99-104:
//   P[t,c] = clean[t,c]^inv_p;  S1[t] = sum_{t' <= t} sum_c P[t',c];  S2[t] = sum_{t' <= t} sum_c mask[t',c] P[t',c]     (float64)
//   ratio[t] = S2[t] > 0 ? S1[t] / S2[t] : 1;  alpha2 = mask ratio (train_nele.py:307);  enh = clean mask^p ratio^p (train_nele.py:137)
//   nele_energy_norm_prefix_fwd / _bwd : siblings of nele_energy_norm_fwd / _bwd (gen.hip), same layouts.
// Arithmetic contract - the operations and order of rt_head_kernel's normalisation, so that bit-equal band features and mask give
// bit-equal alpha2: per frame P = (double)nele_powi_f32(clean, inv_p), the frame's two sums by wave_sum over the 64 bands (one wave per
// frame, lane = band), S1 / S2 accumulated over the frames serially in float64 in frame order, alpha2 = (float)((double)mask * ratio).
// This file is built without FMA contraction (Makefile EXACT), as realtime.hip is: mask * P feeding the first butterfly add must stay a
// product and a sum.
// One workgroup of 1024 threads per utterance, like energy_norm_fwd_kernel: everything stays inside the utterance's rows in a fixed
// order (independent of B and of the batch position).  Frames go in chunks of EP_CH: (1) 16 waves write the chunk's frame sums to LDS,
// (2) two lanes run the two serial float64 scans (T = 501: ~500 dependent adds each), (3) the chunk is applied and packed through the
// 64-frame LDS transpose tile of gen.hip (band features [t][c], D input [c][t][4]: both sides accessed along their contiguous direction).
// Frames behind an utterance's end inside a padded batch are exact zeros: they add +0 to the sums, their D input is zero and their mask
// gradient is zero - no frame counts needed.
#include "common.h"

#define EP_TT 64
#define EP_CH 512

// STD: p = float32(1/6), inv_p = 6 (what every caller passes) as compile-time constants - the same arithmetic with the general pow / powf
// paths of nele_pow_f32 / nele_powi_f32 folded away (they cost the kernel 19 spilled registers)
template <bool STD>
__global__ __launch_bounds__(1024) void energy_norm_prefix_fwd_kernel(const float* __restrict__ clean, const float* __restrict__ mask,
                                                                      const float* __restrict__ noise, float p_, float inv_p_,
                                                                      float* __restrict__ ratio_out, double* __restrict__ s2_out,
                                                                      float* __restrict__ din, float* __restrict__ alpha2, int T) {
    const float p = STD ? (float)(1.0 / 6.0) : p_, inv_p = STD ? 6.0f : inv_p_;
    __shared__ double sp[EP_CH], smp[EP_CH];             // frame sums -> running sums -> (sp) ratio
    __shared__ double carry[2];
    __shared__ float bpl[EP_CH];                          // ratio^p
    __shared__ float te[EP_TT][65], tn[EP_TT][65], tc[EP_TT][65];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const size_t base = (size_t)b * T * 64;
    if (tid < 2) carry[tid] = 0.0;
    for (int c0 = 0; c0 < T; c0 += EP_CH) {
        const int nc = min(EP_CH, T - c0);
        __syncthreads();
        // (1) frame sums: wave wv takes frames wv, wv + 16, ..; four frames' loads in flight
        for (int f0 = wv; f0 < nc; f0 += 64) {
            float cv[4], mv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int f = f0 + 16 * u;
                const size_t g = base + (size_t)(c0 + f) * 64 + lane;
                cv[u] = f < nc ? clean[g] : 0.f;
                mv[u] = f < nc ? mask[g] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int f = f0 + 16 * u;
                if (f < nc) {                                            // (wave-uniform)
                    const double pw = (double)nele_powi_f32(cv[u], inv_p);
                    const double a = wave_sum(pw);
                    const double m = wave_sum((double)mv[u] * pw);
                    if (lane == 0) { sp[f] = a; smp[f] = m; }
                }
            }
        }
        __syncthreads();
        // (2) the serial scans, in frame order: lane 0 S1, lane 1 S2
        if (tid < 2) {
            double* arr = tid ? smp : sp;
            double acc = carry[tid];
            for (int f = 0; f < nc; ++f) {
                acc += arr[f];
                arr[f] = acc;
            }
            carry[tid] = acc;
        }
        __syncthreads();
        if (tid < nc) {
            const double s1 = sp[tid], s2 = smp[tid];
            const double r = s2 > 0.0 ? s1 / s2 : 1.0;
            sp[tid] = r;
            const float rf = (float)r;
            bpl[tid] = nele_pow_f32(rf, p);
            ratio_out[(size_t)b * T + c0 + tid] = rf;
            s2_out[(size_t)b * T + c0 + tid] = s2;
        }
        __syncthreads();
        // (3) apply
        if (!din) {                                       // the enhancement path: alpha2 only, no tiles
            if (alpha2) {
                const int n = nc * 64;
                for (int i = tid; i < n; i += 1024) {
                    const size_t g = base + (size_t)c0 * 64 + i;
                    alpha2[g] = (float)((double)mask[g] * sp[i >> 6]);
                }
            }
            continue;
        }
        for (int t0 = 0; t0 < nc; t0 += EP_TT) {
            const int nt = min(EP_TT, nc - t0);
            __syncthreads();
            float cb[4], mk[4], nz[4];                    // the tile's loads first: one memory round trip, not four
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int idx = tid + 1024 * e, tl = idx >> 6, c = idx & 63;
                const size_t g = base + (size_t)(c0 + t0 + min(tl, nt - 1)) * 64 + c;
                cb[e] = clean[g]; mk[e] = mask[g]; nz[e] = noise[g];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int idx = tid + 1024 * e, tl = idx >> 6, c = idx & 63;
                if (tl < nt) {
                    if (alpha2) alpha2[base + (size_t)(c0 + t0 + tl) * 64 + c] = (float)((double)mk[e] * sp[t0 + tl]);
                    te[tl][c] = cb[e] * nele_pow_f32(mk[e], p) * bpl[t0 + tl];
                    tn[tl][c] = nz[e];
                    tc[tl][c] = cb[e];
                }
            }
            __syncthreads();
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int idx = tid + 1024 * e, c = idx >> 6, tl = idx & 63;
                if (tl < nt)
                    *reinterpret_cast<float4*>(din + (((size_t)b * 64 + c) * T + c0 + t0 + tl) * 4) = make_float4(te[tl][c], tn[tl][c], tc[tl][c], 0.f);
            }
        }
    }
}

// dmask from d(din): only channel 0 (enh) depends on the mask.  With dE = ddin[..., 0], bp[t] = ratio[t]^p,
//   R[t] = sum_c dE[t,c] clean[t,c] mask[t,c]^p,  w[t] = R[t] p bp[t] / S2[t] (0 where S2[t] <= 0: ratio is the constant 1 there),
//   K[t] = sum_{t'' >= t} w[t'']   (S2[t''] holds mask[t,c] P[t,c] for every t'' >= t: a SUFFIX sum)
//   dmask[t,c] = dE clean p mask^(p-1) bp[t]  -  K[t] clean^inv_p
// Chunks of EP_CH frames from the LAST one down (K carries from the later chunk).  As in energy_norm_bwd_kernel, with the forward pass's
// D input at hand enh is read back: clean mask^p = enh / bp and clean mask^(p-1) bp = enh / mask (one pow per element instead of four).
template <bool STD>
__global__ __launch_bounds__(1024) void energy_norm_prefix_bwd_kernel(const float* __restrict__ clean, const float* __restrict__ mask,
                                                                      const float* __restrict__ ratio_in, const double* __restrict__ s2_in,
                                                                      const float* __restrict__ ddin, const float* __restrict__ din, float p_,
                                                                      float inv_p_, float* __restrict__ dmask, int T) {
    const float p = STD ? (float)(1.0 / 6.0) : p_, inv_p = STD ? 6.0f : inv_p_;
    __shared__ double kw[EP_CH];                          // w[t] -> K[t]
    __shared__ double kcarry;
    __shared__ float bpl[EP_CH];
    __shared__ float td[EP_TT][65], te[EP_TT][65];
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t base = (size_t)b * T * 64;
    if (tid == 0) kcarry = 0.0;
    const int nchunks = (T + EP_CH - 1) / EP_CH;
    for (int ch = nchunks - 1; ch >= 0; --ch) {
        const int c0 = ch * EP_CH, nc = min(EP_CH, T - c0);
        __syncthreads();
        if (tid < nc) bpl[tid] = nele_pow_f32(ratio_in[(size_t)b * T + c0 + tid], p);
        for (int pass = 0; pass < 2; ++pass) {
            if (pass == 1) {
                __syncthreads();
                if (tid < nc) {
                    const double s2 = s2_in[(size_t)b * T + c0 + tid];
                    kw[tid] = s2 > 0.0 ? kw[tid] * (double)p * (double)bpl[tid] / s2 : 0.0;
                }
                __syncthreads();
                if (tid == 0) {                           // the serial suffix scan, from the chunk's last frame down
                    double acc = kcarry;
                    for (int f = nc - 1; f >= 0; --f) {
                        acc += kw[f];
                        kw[f] = acc;
                    }
                    kcarry = acc;
                }
            }
            for (int t0 = 0; t0 < nc; t0 += EP_TT) {
                const int nt = min(EP_TT, nc - t0);
                __syncthreads();
#pragma unroll
                for (int e = 0; e < 4; ++e) {                       // dE (and enh) of the tile, read along t (contiguous in [c][t][4])
                    const int idx = tid + 1024 * e, c = idx >> 6, tl = idx & 63;
                    if (tl < nt) {
                        const size_t g = (((size_t)b * 64 + c) * T + c0 + t0 + tl) * 4;
                        td[tl][c] = ddin[g];
                        if (din) te[tl][c] = din[g];
                    }
                }
                __syncthreads();
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int idx = tid + 1024 * e, tl = idx >> 6, c = idx & 63;     // a wave = one frame, lane = band
                    if (tl < nt) {                                                     // (wave-uniform)
                        const size_t g = base + (size_t)(c0 + t0 + tl) * 64 + c;
                        const float dE = td[tl][c], bp = bpl[t0 + tl];
                        if (pass == 0) {
                            const float v = din ? dE * (te[tl][c] / bp) : dE * clean[g] * nele_pow_f32(mask[g], p);
                            const double r = wave_sum((double)v);
                            if (c == 0) kw[t0 + tl] = r;
                        } else {
                            const float k = (float)kw[t0 + tl];
                            const float cb = clean[g], m = mask[g];
                            // (a zero band feature - frames behind an utterance's end - gives an exact zero whatever the mask is)
                            const float a = din ? dE * p * (te[tl][c] / m) : dE * cb * p * powf(m, p - 1.f) * bp;
                            dmask[g] = a - k * nele_powi_f32(cb, inv_p);
                        }
                    }
                }
            }
        }
    }
}

extern "C" int nele_energy_norm_prefix_fwd(const float* clean, const float* mask, const float* noise, float p, float inv_p, float* ratio,
                                           double* s2, float* din, float* alpha2, int B, int T, void* stream) {
    NELE_CHECK_ARG(clean && mask && ratio && s2 && B > 0 && T > 0, "nele_energy_norm_prefix_fwd: bad arguments");
    NELE_CHECK_ARG(!din || noise, "nele_energy_norm_prefix_fwd: din requested without noise features");
    if (p == (float)(1.0 / 6.0) && inv_p == 6.0f)
        hipLaunchKernelGGL(energy_norm_prefix_fwd_kernel<true>, dim3(B), dim3(1024), 0, as_stream(stream), clean, mask, noise, p, inv_p, ratio, s2,
                           din, alpha2, T);
    else
        hipLaunchKernelGGL(energy_norm_prefix_fwd_kernel<false>, dim3(B), dim3(1024), 0, as_stream(stream), clean, mask, noise, p, inv_p, ratio, s2,
                           din, alpha2, T);
    NELE_CHECK_LAUNCH("nele_energy_norm_prefix_fwd");
    return NELE_OK;
}

extern "C" int nele_energy_norm_prefix_bwd(const float* clean, const float* mask, const float* ratio, const double* s2, const float* ddin,
                                           const float* din, float p, float inv_p, float* dmask, int B, int T, void* stream) {
    NELE_CHECK_ARG(clean && mask && ratio && s2 && ddin && dmask && B > 0 && T > 0, "nele_energy_norm_prefix_bwd: bad arguments");
    if (p == (float)(1.0 / 6.0) && inv_p == 6.0f)
        hipLaunchKernelGGL(energy_norm_prefix_bwd_kernel<true>, dim3(B), dim3(1024), 0, as_stream(stream), clean, mask, ratio, s2, ddin, din, p,
                           inv_p, dmask, T);
    else
        hipLaunchKernelGGL(energy_norm_prefix_bwd_kernel<false>, dim3(B), dim3(1024), 0, as_stream(stream), clean, mask, ratio, s2, ddin, din, p,
                           inv_p, dmask, T);
    NELE_CHECK_LAUNCH("nele_energy_norm_prefix_bwd");
    return NELE_OK;
}
