// fd_scan_bwd_core.h -- the per-(row, state) arithmetic of the two selective-scan backwards (fd_scan_bwd.hip, fd_cross_scan_bwd.hip),
// once.  A tile is one wave's span: 64 lanes x E consecutive positions.  Nothing of the forward is stored: the h and the g = dL/dh
// of every position are recomputed from tile carries, in three launches:
//   carry: sbc_fold + sbc_compose0 leave per (row, tile, state) the tile's composite Pa = prod a, its local end state H (from
//          h = 0) and its local reverse composite G (the a_{t0} g_{t0} the tile hands to its predecessor, from a zero carry);
//   chain: scan_bwd_chain_kernel turns H into each tile's carry-in h and G into its carry-in g, sequentially per (row, state);
//   main:  sbc_fold + sbc_carry_in + sbc_replay replay h forward and g backward inside the tile and accumulate the gradients.
// What differs between the two files stays in them: operand staging, state chunking, dt's recomputation, the layout of the
// workspace and every launch.  Conventions of fd_train_common.h: anonymous namespace, `template <int = 0>` on what a file may not
// launch.  (The 64-lane sum both backwards use is wave_sum of fd_common.h.)
#pragma once
#include "fd_train_common.h"

namespace {

// d softplus(v) / dv, 1 above softplus's threshold of 20
__device__ __forceinline__ float sbc_softplus_grad(float v) { return v > 20.0f ? 1.f : 1.f / (1.f + __expf(-v)); }

// One step of an affine recurrence x -> a x + b whose offset b is itself a product (dt B u forward, dy C backward).  The compiler
// may contract either product into the sum, and where both have as many uses the choice hung on the order in which the two
// operands reached it.  Spelled out: b rounded, a x fused.
__device__ __forceinline__ float sbc_step(float a, float x, float b) { return __builtin_fmaf(a, x, b); }

// A lane's E positions as one affine map each way: a_t = exp(dt_t A), hv_t = dt_t B_t u_t (the forward map's offset),
// forward h -> Pa h + Pb over the positions in order, reverse x -> Pa x + Qb from the last position back (x = a_{t+1} g_{t+1}).
// dt = 0 (past the end) is the identity map.
template <int E>
__device__ __forceinline__ void sbc_fold(const float (&dt)[E], float An, const float (&Bv)[E], const float (&Cv)[E],
                                         const float (&uu)[E], const float (&dy)[E], float (&a)[E], float (&hv)[E], float &Pa,
                                         float &Pb, float &Qb) {
    Pa = 1.f, Pb = 0.f;
#pragma unroll
    for (int i = 0; i < E; ++i) {
        a[i] = __expf(dt[i] * An);
        hv[i] = dt[i] * Bv[i] * uu[i];
        Pb = sbc_step(a[i], Pb, hv[i]);
        Pa = a[i] * Pa;
    }
    float q = dy[E - 1] * Cv[E - 1] + 0.f;
#pragma unroll
    for (int i = E - 2; i >= 0; --i) q = sbc_step(a[i + 1], q, dy[i] * Cv[i]);
    Qb = a[0] * q;
}

// lane 0 composes lanes [0, 2o) from [0, o) and [o, 2o): forward map 1 then 2, reverse map 2 then 1.  Lane 0 ends with the tile's.
__device__ __forceinline__ void sbc_compose0(float &Pa, float &Pb, float &Qb) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float pa = __shfl_down(Pa, o, 64), pb = __shfl_down(Pb, o, 64), qb = __shfl_down(Qb, o, 64);
        Pb = pa * Pb + pb;
        Qb = Pa * qb + Qb;
        Pa = Pa * pa;
    }
}

// Inclusive scans over the wave, forward over the lanes before and reverse over the lanes after, shifted by one lane to exclusive
// ones and applied to the tile's carries: h = the state entering this lane's first position, X = a_{t+1} g_{t+1} after its last.
__device__ __forceinline__ void sbc_carry_in(int lane, float Pa, float Pb, float Qb, float hin, float gin, float &h, float &X) {
    float fa = Pa, fb = Pb, ra = Pa, rb = Qb;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float pa = __shfl_up(fa, o, 64), pb = __shfl_up(fb, o, 64);
        const float qa = __shfl_down(ra, o, 64), qb = __shfl_down(rb, o, 64);
        if (lane >= o) {
            fb = fa * pb + fb;
            fa = fa * pa;
        }
        if (lane + o < 64) {
            rb = ra * qb + rb;
            ra = ra * qa;
        }
    }
    float ea = __shfl_up(fa, 1, 64), eb = __shfl_up(fb, 1, 64);
    float xa = __shfl_down(ra, 1, 64), xb = __shfl_down(rb, 1, 64);
    if (lane == 0) ea = 1.f, eb = 0.f;
    if (lane == 63) xa = 1.f, xb = 0.f;
    h = ea * hin + eb;
    X = xa * gin + xb;
}

// h forward, then g backward: accC += dy h (dC), accB += g dt u (dB), gu += g dt B (du), gt += g (B u + A a h_{t-1}) (ddt),
// pA += g dt a h_{t-1} (dA).  a, hv: sbc_fold's; h, X: sbc_carry_in's.
template <int E>
__device__ __forceinline__ void sbc_replay(const float (&dt)[E], float An, const float (&Bv)[E], const float (&Cv)[E],
                                           const float (&uu)[E], const float (&dy)[E], const float (&a)[E], float (&hv)[E], float h,
                                           float X, float (&accB)[E], float (&accC)[E], float (&gu)[E], float (&gt)[E], float &pA) {
    float hp[E];
#pragma unroll
    for (int i = 0; i < E; ++i) {
        hp[i] = h;
        h = a[i] * h + hv[i];
        hv[i] = h;                                           // b_t so far, h_t from here
    }
    float gi = dy[E - 1] * Cv[E - 1] + X;
#pragma unroll
    for (int i = E - 1; i >= 0; --i) {
        if (i < E - 1) gi = sbc_step(a[i + 1], gi, dy[i] * Cv[i]);
        X = a[i] * gi;
        const float gdt = gi * dt[i], w = X * hp[i];         // w = g a h_{t-1}
        accC[i] += dy[i] * hv[i];
        accB[i] += gdt * uu[i];
        gu[i] += gdt * Bv[i];
        gt[i] += gi * Bv[i] * uu[i] + An * w;
        pA += dt[i] * w;
    }
}

// ---- the carries: H -> h entering tile j, G -> a_{t+1} g_{t+1} entering tile j from its end --------------------------------------
// ws_pa / ws_h / ws_g: [tile][RN], RN = rows x states
template <int = 0>
__global__ __launch_bounds__(256) void scan_bwd_chain_kernel(const float *__restrict__ ws_pa, float *__restrict__ ws_h,
                                                            float *__restrict__ ws_g, int64_t RN, int ntiles) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= RN) return;
    float h = 0.f;
    for (int j = 0; j < ntiles; ++j) {
        const int64_t k = (int64_t)j * RN + i;
        const float a = ws_pa[k], hb = ws_h[k];
        ws_h[k] = h;
        h = a * h + hb;
    }
    float x = 0.f;
    for (int j = ntiles - 1; j >= 0; --j) {
        const int64_t k = (int64_t)j * RN + i;
        const float a = ws_pa[k], gb = ws_g[k];
        ws_g[k] = x;
        x = a * x + gb;
    }
}

template <int = 0>
void scan_bwd_chain_launch(const float *ws_pa, float *ws_h, float *ws_g, int64_t RN, int ntiles, hipStream_t st) {
    hipLaunchKernelGGL(scan_bwd_chain_kernel<>, dim3((unsigned)((RN + 255) / 256)), dim3(256), 0, st, ws_pa, ws_h, ws_g, RN, ntiles);
}

}  // namespace
