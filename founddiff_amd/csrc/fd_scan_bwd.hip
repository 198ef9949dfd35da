// fd_scan_bwd.hip -- the backward of fd_selective_scan_fwd_f32 (fd_scan_ref.hip), i.e. of the reference extension's
//     selective_scan_cuda_core.bwd(u, delta, A, B, C, D, delta_bias, dout, x, delta_softplus, nrows)
// in the same operand layout: fp32, L contiguous; u / delta / dout (b, KD, L); A (KD, N); B / C (b, K, N, L);
// D / delta_bias (KD) or null; channel d reads group g = d / (KD / K).
//
//     dt_t = softplus(delta_t + bias) (or without softplus),  a_t = exp(dt_t A),  h_t = a_t h_{t-1} + dt_t B_t u_t
//     g_t  = dL/dh_t = dout_t C_t + a_{t+1} g_{t+1}                          (the reverse affine recurrence)
//     dC = sum_{d in g} dout h          dB = sum_{d in g} g dt u          du = D dout + sum_n g dt B
//     ddt = sum_n g (B u + A a h_{t-1}) ddelta = ddt * sigmoid(delta + bias) (softplus, below its threshold of 20)
//     dA[d,n] = sum_{b,t} g dt a h_{t-1}   dD[d] = sum_{b,t} dout u   ddelta_bias[d] = sum_{b,t} ddelta
//
// Nothing of the forward is stored: the h and g of every position are recomputed from tile carries by the shared core,
// fd_scan_bwd_core.h.  A tile is one wave's span, 64 lanes x 4 consecutive positions.  Four launches (plus one when the rows of a
// group are split):
//   1. carry:  per (row, tile, n) the tile's composites (the core's fold and lane-0 composition);
//   2. chain:  the core's chain kernel;
//   3. main:   per (batch, group, tile, row split) a workgroup of 4 waves walks the split's rows, wave w taking every fourth,
//              replays h forward and g backward inside the tile (the core's carry-in and replay), writes du and ddelta per row, keeps dB
//              and dC of the tile in registers and sums the four waves through LDS in a fixed order; per (row, tile) partials
//              of dA, dD and ddelta_bias go to the workspace.  Rows are split over workgroups only where (batch, group,
//              tile) alone would leave the chip idle (the deep levels: L = 1024, up to 1024 rows per group); the splits
//              then write dB / dC partials that launch 5 sums in split order;
//   4. params: one workgroup per channel sums the dA / dD / ddelta_bias partials over (batch, tile) in a fixed order.
// No float atomics anywhere: two calls on the same inputs give the same bits.  States beyond NC = 4 / 8 are walked in
// chunks of NC; du and the un-scaled ddt then accumulate in place over the chunks (same lane, same addresses).
#include "fd_scan_bwd_core.h"

namespace {

constexpr int SB_E = 4, SB_TILE = 64 * SB_E, SB_T = 256, SB_W = SB_T / 64;

__device__ __forceinline__ void sb_load4(const float *p, int64_t l0, int64_t L, bool vec, float (&v)[SB_E]) {
    if (vec && l0 + SB_E <= L) {
        const f32x4 q = *(const f32x4 *)(p + l0);
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
    } else {
#pragma unroll
        for (int i = 0; i < SB_E; ++i) v[i] = l0 + i < L ? p[l0 + i] : 0.f;
    }
}

__device__ __forceinline__ void sb_store4(float *p, int64_t l0, int64_t L, bool vec, const float (&v)[SB_E]) {
    if (vec && l0 + SB_E <= L) {
        *(f32x4 *)(p + l0) = (f32x4){v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int i = 0; i < SB_E; ++i)
            if (l0 + i < L) p[l0 + i] = v[i];
    }
}

// dt of 4 positions (0 past the end: the identity map a = 1, b = 0) and d dt / d delta
__device__ __forceinline__ void sb_dt(const float (&dl)[SB_E], float bias, int softplus, int64_t l0, int64_t L,
                                      float (&dt)[SB_E], float (&fac)[SB_E]) {
#pragma unroll
    for (int i = 0; i < SB_E; ++i) {
        const float v = dl[i] + bias;
        float t = v, f = 1.f;
        if (softplus) {
            t = fd_softplus(v);
            f = sbc_softplus_grad(v);
        }
        dt[i] = l0 + i < L ? t : 0.f;
        fac[i] = f;
    }
}

// ---- 1. tile composites -------------------------------------------------------------------------------------------
// ws_pa / ws_h / ws_g: [tile][row][n]
__global__ __launch_bounds__(SB_T) void scan_bwd_carry_kernel(const float *__restrict__ u, const float *__restrict__ delta,
                                                             const float *__restrict__ A, const float *__restrict__ Bm,
                                                             const float *__restrict__ Cm, const float *__restrict__ dbias,
                                                             const float *__restrict__ dout, int softplus,
                                                             float *__restrict__ ws_pa, float *__restrict__ ws_h,
                                                             float *__restrict__ ws_g, int KD, int K, int N, int64_t L,
                                                             int ntiles, int64_t rows) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tgroups = (ntiles + SB_W - 1) / SB_W;
    const int64_t row = blockIdx.x / tgroups;
    const int tile = (int)(blockIdx.x - row * tgroups) * SB_W + wave;
    if (tile >= ntiles) return;
    const int b = (int)(row / KD), d = (int)(row - (int64_t)b * KD);
    const int g = d / (KD / K);
    const bool vec = (L & 3) == 0;
    const int64_t l0 = (int64_t)tile * SB_TILE + lane * SB_E;
    const float *Bg = Bm + ((int64_t)b * K + g) * N * L, *Cg = Cm + ((int64_t)b * K + g) * N * L;
    float uu[SB_E], dl[SB_E], dy[SB_E], dt[SB_E], fac[SB_E];
    sb_load4(u + row * L, l0, L, vec, uu);
    sb_load4(delta + row * L, l0, L, vec, dl);
    sb_load4(dout + row * L, l0, L, vec, dy);
    sb_dt(dl, dbias ? dbias[d] : 0.f, softplus, l0, L, dt, fac);
    for (int n = 0; n < N; ++n) {
        const float An = A[(int64_t)d * N + n];
        float Bv[SB_E], Cv[SB_E], a[SB_E], hv[SB_E], Pa, Pb, Qb;
        sb_load4(Bg + (int64_t)n * L, l0, L, vec, Bv);
        sb_load4(Cg + (int64_t)n * L, l0, L, vec, Cv);
        sbc_fold(dt, An, Bv, Cv, uu, dy, a, hv, Pa, Pb, Qb);
        // this kernel's H has been rounded as fma(dt B, u, a H) since it was written, not as the core's fma(a, H, dt B u): kept
        Pb = 0.f;
#pragma unroll
        for (int i = 0; i < SB_E; ++i) Pb = __builtin_fmaf(dt[i] * Bv[i], uu[i], a[i] * Pb);
        sbc_compose0(Pa, Pb, Qb);
        if (lane == 0) {
            const int64_t k = ((int64_t)tile * rows + row) * N + n;
            ws_pa[k] = Pa;
            ws_h[k] = Pb;
            ws_g[k] = Qb;
        }
    }
}

// ---- 3. the gradients ---------------------------------------------------------------------------------------------------
// dBo / dCo: [split][b][K][N][L] (split 0 = the outputs themselves when S == 1); part: [N + 2][KD][b][tile]
template <int NC>
__global__ __launch_bounds__(SB_T) void scan_bwd_main_kernel(
    const float *__restrict__ u, const float *__restrict__ delta, const float *__restrict__ A, const float *__restrict__ Bm,
    const float *__restrict__ Cm, const float *__restrict__ Dv, const float *__restrict__ dbias, const float *__restrict__ dout,
    int softplus, float *__restrict__ du, float *__restrict__ ddelta, float *__restrict__ dBo, float *__restrict__ dCo,
    const float *__restrict__ hin, const float *__restrict__ gin, float *__restrict__ part, int batch, int KD, int K, int N,
    int64_t L, int ntiles, int S) {
    __shared__ float s_red[SB_W - 1][2][SB_TILE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile = (int)(blockIdx.x % ntiles);
    const int rest = (int)(blockIdx.x / ntiles);
    const int s = rest % S, bg = rest / S;
    const int b = bg / K, g = bg - b * K;
    const int Dg = KD / K;
    const int r0 = (int)((int64_t)Dg * s / S), r1 = (int)((int64_t)Dg * (s + 1) / S);
    const int64_t rows = (int64_t)batch * KD, M = (int64_t)batch * ntiles;
    const bool vec = (L & 3) == 0;
    const int64_t l0 = (int64_t)tile * SB_TILE + lane * SB_E;
    const float *Bg = Bm + (int64_t)bg * N * L, *Cg = Cm + (int64_t)bg * N * L;
    float *dBs = dBo + ((int64_t)s * batch * K + bg) * N * L, *dCs = dCo + ((int64_t)s * batch * K + bg) * N * L;
    for (int n0 = 0; n0 < N; n0 += NC) {
        const bool first = n0 == 0, last = n0 + NC >= N;
        float accB[NC][SB_E], accC[NC][SB_E];
#pragma unroll
        for (int j = 0; j < NC; ++j)
#pragma unroll
            for (int i = 0; i < SB_E; ++i) accB[j][i] = accC[j][i] = 0.f;
        for (int dd = r0 + wave; dd < r1; dd += SB_W) {
            const int d = g * Dg + dd;
            const int64_t row = (int64_t)b * KD + d;
            float uu[SB_E], dl[SB_E], dy[SB_E], dt[SB_E], fac[SB_E], gu[SB_E], gt[SB_E];
            sb_load4(u + row * L, l0, L, vec, uu);
            sb_load4(delta + row * L, l0, L, vec, dl);
            sb_load4(dout + row * L, l0, L, vec, dy);
            sb_dt(dl, dbias ? dbias[d] : 0.f, softplus, l0, L, dt, fac);
            if (first) {
                const float Dd = Dv ? Dv[d] : 0.f;
#pragma unroll
                for (int i = 0; i < SB_E; ++i) gu[i] = Dd * dy[i], gt[i] = 0.f;
            } else {                                         // the chunks before this one left du and the un-scaled ddt
                sb_load4(du + row * L, l0, L, vec, gu);
                sb_load4(ddelta + row * L, l0, L, vec, gt);
            }
            float pA[NC];
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                pA[j] = 0.f;
                const int n = n0 + j;
                if (n >= N) continue;
                const float An = A[(int64_t)d * N + n];
                float Bv[SB_E], Cv[SB_E], a[SB_E], hv[SB_E], Pa, Pb, Qb, h, X;
                sb_load4(Bg + (int64_t)n * L, l0, L, vec, Bv);
                sb_load4(Cg + (int64_t)n * L, l0, L, vec, Cv);
                sbc_fold(dt, An, Bv, Cv, uu, dy, a, hv, Pa, Pb, Qb);
                const int64_t k = ((int64_t)tile * rows + row) * N + n;
                sbc_carry_in(lane, Pa, Pb, Qb, hin[k], gin[k], h, X);
                sbc_replay(dt, An, Bv, Cv, uu, dy, a, hv, h, X, accB[j], accC[j], gu, gt, pA[j]);
            }
            float pD = 0.f, pBias = 0.f;
            if (first)
#pragma unroll
                for (int i = 0; i < SB_E; ++i) pD += dy[i] * uu[i];
            if (last)
#pragma unroll
                for (int i = 0; i < SB_E; ++i) {
                    gt[i] *= fac[i];
                    if (l0 + i < L) pBias += gt[i];
                }
            sb_store4(du + row * L, l0, L, vec, gu);
            sb_store4(ddelta + row * L, l0, L, vec, gt);
            const int64_t pk = ((int64_t)d * batch + b) * ntiles + tile, qs = (int64_t)KD * M;
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                if (n0 + j >= N) continue;
                const float v = wave_sum(pA[j]);
                if (lane == 0) part[(n0 + j) * qs + pk] = v;
            }
            if (first) {
                const float v = wave_sum(pD);
                if (lane == 0) part[N * qs + pk] = v;
            }
            if (last) {
                const float v = wave_sum(pBias);
                if (lane == 0) part[(N + 1) * qs + pk] = v;
            }
        }
        // dB / dC of the tile: wave 0 + wave 1 + wave 2 + wave 3
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            if (n0 + j >= N) continue;
            if (wave > 0)
#pragma unroll
                for (int i = 0; i < SB_E; ++i) {
                    s_red[wave - 1][0][lane * SB_E + i] = accB[j][i];
                    s_red[wave - 1][1][lane * SB_E + i] = accC[j][i];
                }
            __syncthreads();
            if (wave == 0) {
                float vb[SB_E], vc[SB_E];
#pragma unroll
                for (int i = 0; i < SB_E; ++i) {
                    vb[i] = accB[j][i];
                    vc[i] = accC[j][i];
#pragma unroll
                    for (int w = 0; w < SB_W - 1; ++w) {
                        vb[i] += s_red[w][0][lane * SB_E + i];
                        vc[i] += s_red[w][1][lane * SB_E + i];
                    }
                }
                sb_store4(dBs + (int64_t)(n0 + j) * L, l0, L, vec, vb);
                sb_store4(dCs + (int64_t)(n0 + j) * L, l0, L, vec, vc);
            }
            __syncthreads();
        }
    }
}

// ---- 4. dA / dD / ddelta_bias: one workgroup per channel, partials over (batch, tile) in a fixed order ------------------
__global__ __launch_bounds__(SB_T) void scan_bwd_param_kernel(const float *__restrict__ part, int KD, int N, int64_t M,
                                                             float *__restrict__ dA, float *__restrict__ dD,
                                                             float *__restrict__ dbias) {
    __shared__ float s[SB_T];
    const int tid = threadIdx.x, d = blockIdx.x;
    for (int q = 0; q < N + 2; ++q) {
        float *dst = q < N ? dA + (int64_t)d * N + q : q == N ? (dD ? dD + d : nullptr) : (dbias ? dbias + d : nullptr);
        if (!dst) continue;
        const float *p = part + ((int64_t)q * KD + d) * M;
        float v = 0.f;
        for (int64_t m = tid; m < M; m += SB_T) v += p[m];
        s[tid] = v;
        __syncthreads();
        for (int o = SB_T / 2; o > 0; o >>= 1) {
            if (tid < o) s[tid] += s[tid + o];
            __syncthreads();
        }
        if (tid == 0) *dst = s[0];
        __syncthreads();
    }
}

// ---- 5. dB / dC over the row splits, in split order ---------------------------------------------------------------------
__global__ __launch_bounds__(SB_T) void scan_bwd_bc_kernel(const float *__restrict__ pB, const float *__restrict__ pC,
                                                          int S, int64_t tot, float *__restrict__ dB, float *__restrict__ dC) {
    const int64_t i = (int64_t)blockIdx.x * SB_T + threadIdx.x;
    if (i >= tot) return;
    float vb = 0.f, vc = 0.f;
    for (int s = 0; s < S; ++s) {
        vb += pB[(int64_t)s * tot + i];
        vc += pC[(int64_t)s * tot + i];
    }
    dB[i] = vb;
    dC[i] = vc;
}

int sb_ntiles(int64_t L) { return (int)((L + SB_TILE - 1) / SB_TILE); }

// row splits per (batch, group, tile): enough workgroups to fill the chip, at least 16 rows (4 per wave) per split
int sb_splits(int batch, int KD, int K, int64_t L) {
    const int64_t wg = (int64_t)batch * K * sb_ntiles(L);
    const int Dg = KD / K;
    int S = 1;
    while (wg * S < 1024 && S * 2 * 16 <= Dg) S *= 2;
    return S;
}

struct SbLayout {
    int ntiles, tgroups, S, NC;           // tiles, carry workgroups per row (SB_W tiles each), row splits, states per main-kernel chunk
    int64_t comp, part, bc, total;        // floats: each of the 3 composite arrays, the parameter partials, each dB / dC slab set
};

SbLayout sb_layout(int batch, int KD, int K, int N, int64_t L) {
    SbLayout w;
    w.ntiles = sb_ntiles(L);
    w.tgroups = (w.ntiles + SB_W - 1) / SB_W;
    w.S = sb_splits(batch, KD, K, L);
    w.NC = N <= 4 ? 4 : 8;
    w.comp = round4((int64_t)w.ntiles * batch * KD * N);
    w.part = round4((int64_t)(N + 2) * KD * batch * w.ntiles);
    w.bc = w.S > 1 ? round4((int64_t)w.S * batch * K * N * L) : 0;
    w.total = 3 * w.comp + w.part + 2 * w.bc;
    return w;
}

// the shape checks of the call, shared with fd_selective_scan_bwd_geom
int sb_shape(const char *name, int nrows, int batch, int KD, int K, int N, int64_t L) {
    FD_REQUIRE(nrows >= 1 && nrows <= 4, "%s: nrows=%d not in 1..4", name, nrows);
    FD_REQUIRE(batch > 0 && KD > 0 && K > 0 && L > 0 && KD % (K * nrows) == 0,
               "%s: u.shape[1]=%d must be a multiple of B.shape[1]*nrows=%d*%d", name, KD, K, nrows);
    FD_REQUIRE(N >= 1 && N <= 256, "%s: d_state=%d not in 1..256", name, N);
    return FD_OK;
}

}  // namespace

extern "C" int64_t fd_selective_scan_bwd_ws_floats(int batch, int KD, int K, int N, int64_t L) {
    if (batch <= 0 || KD <= 0 || K <= 0 || N <= 0 || L <= 0 || KD % K) return 0;
    return sb_layout(batch, KD, K, N, L).total;
}

// What fd_selective_scan_bwd_f32 launches for this shape: sb_layout's own values, host only (tests/scan_bwd_cases.py).
extern "C" int fd_selective_scan_bwd_geom(int batch, int KD, int K, int N, int64_t L, int32_t out[8]) {
    FD_REQUIRE(out, "fd_selective_scan_bwd_geom: null pointer");
    for (int i = 0; i < 8; ++i) out[i] = 0;
    if (int rc = sb_shape("fd_selective_scan_bwd_geom", 1, batch, KD, K, N, L)) return rc;
    const SbLayout w = sb_layout(batch, KD, K, N, L);
    const int Dg = KD / K;
    out[0] = w.ntiles;
    out[1] = w.tgroups;
    out[2] = (int32_t)(L - (int64_t)(w.ntiles - 1) * SB_TILE);
    out[3] = w.S;
    out[4] = w.NC;
    out[5] = (Dg + w.S - 1) / w.S;          // rows of the largest split: split s walks rows [Dg s / S, Dg (s + 1) / S) of its group
    out[6] = Dg;
    return FD_OK;
}

extern "C" int fd_selective_scan_bwd_f32(const float *u, const float *delta, const float *A, const float *B, const float *C,
                                         const float *D, const float *delta_bias, const float *dout, int delta_softplus,
                                         int nrows, int batch, int KD, int K, int N, int64_t L, float *du, float *ddelta,
                                         float *dA, float *dB, float *dC, float *dD, float *ddelta_bias, float *ws,
                                         void *stream) {
    FD_REQUIRE(u && delta && A && B && C && dout && du && ddelta && dA && dB && dC && ws,
               "fd_selective_scan_bwd_f32: null pointer");
    FD_REQUIRE(!D == !dD, "fd_selective_scan_bwd_f32: dD must be given exactly when D is");
    FD_REQUIRE(!delta_bias == !ddelta_bias, "fd_selective_scan_bwd_f32: ddelta_bias must be given exactly when delta_bias is");
    if (int rc = sb_shape("fd_selective_scan_bwd_f32", nrows, batch, KD, K, N, L)) return rc;
    FD_REQUIRE((((uintptr_t)u | (uintptr_t)delta | (uintptr_t)B | (uintptr_t)C | (uintptr_t)dout | (uintptr_t)du |
                 (uintptr_t)ddelta | (uintptr_t)dB | (uintptr_t)dC | (uintptr_t)ws) & 15) == 0,
               "fd_selective_scan_bwd_f32: tensors must be 16-byte aligned");
    const SbLayout w = sb_layout(batch, KD, K, N, L);
    const hipStream_t st = (hipStream_t)stream;
    const int64_t rows = (int64_t)batch * KD, RN = rows * N;
    float *pa = ws, *hh = ws + w.comp, *gg = ws + 2 * w.comp, *part = ws + 3 * w.comp;
    float *pB = w.S > 1 ? part + w.part : dB, *pC = w.S > 1 ? part + w.part + w.bc : dC;
    hipLaunchKernelGGL(scan_bwd_carry_kernel, dim3((unsigned)(rows * w.tgroups)), dim3(SB_T), 0, st, u, delta, A, B, C,
                       delta_bias, dout, delta_softplus, pa, hh, gg, KD, K, N, L, w.ntiles, rows);
    FD_LAUNCH_OK("fd_selective_scan_bwd_f32 (carry)");
    scan_bwd_chain_launch(pa, hh, gg, RN, w.ntiles, st);
    FD_LAUNCH_OK("fd_selective_scan_bwd_f32 (chain)");
    const dim3 grid((unsigned)((int64_t)batch * K * w.S * w.ntiles));
    if (w.NC == 4)
        hipLaunchKernelGGL(scan_bwd_main_kernel<4>, grid, dim3(SB_T), 0, st, u, delta, A, B, C, D, delta_bias, dout,
                           delta_softplus, du, ddelta, pB, pC, hh, gg, part, batch, KD, K, N, L, w.ntiles, w.S);
    else
        hipLaunchKernelGGL(scan_bwd_main_kernel<8>, grid, dim3(SB_T), 0, st, u, delta, A, B, C, D, delta_bias, dout,
                           delta_softplus, du, ddelta, pB, pC, hh, gg, part, batch, KD, K, N, L, w.ntiles, w.S);
    FD_LAUNCH_OK("fd_selective_scan_bwd_f32 (main)");
    hipLaunchKernelGGL(scan_bwd_param_kernel, dim3((unsigned)KD), dim3(SB_T), 0, st, part, KD, N, (int64_t)batch * w.ntiles,
                       dA, dD, ddelta_bias);
    FD_LAUNCH_OK("fd_selective_scan_bwd_f32 (params)");
    if (w.S > 1) {
        const int64_t tot = (int64_t)batch * K * N * L;
        hipLaunchKernelGGL(scan_bwd_bc_kernel, dim3((unsigned)((tot + SB_T - 1) / SB_T)), dim3(SB_T), 0, st, pB, pC, w.S,
                           tot, dB, dC);
        FD_LAUNCH_OK("fd_selective_scan_bwd_f32 (dB / dC splits)");
    }
    return FD_OK;
}
