// fd_adaln_train.hip -- the element-wise frame of the reference's Mamba_block (src/DADiff.py:477-488) for training, fp32, NHWC:
//
//   fd_adaln_fwd_f32      out = LN(x) * (1 + scale[b]) + shift[b]             (norm1 / norm2 + modulate; mean, rstd kept per pixel)
//   fd_adaln_bwd_f32      its backward, the residual path's gradient added to dx in the same pass
//   fd_gate_res_fwd_f32   out = x + gate[b] * y                               (the gated residual add)
//   fd_gate_res_bwd_f32   dy = gate[b] * dout, dgate = sum_hw dout * y        (dx IS dout: nothing to write)
//
// shift, scale and gate are the chunks of adaLN_modulation's (B, 6C) output, read in place through a row stride; their gradients
// are written through a row stride in the same way.
//
// Rows: a group of lpr = 16 / 32 / 64 lanes owns one pixel, a lane VPL = 1 or 2 16-byte vectors of it (channel 4 (j lpr + sub)),
// so a workgroup of 256 threads takes 256 / lpr pixels at a time and a row's sums are shuffles inside one wave.  The statistics
// are centred: the mean first, then the variance of the centred row held in registers.  Every tensor is read once and written
// once: the forwards move 2 resp. 3 tensors, fd_adaln_bwd_f32 3 or 4 (dres), fd_gate_res_bwd_f32 3.
//
// Backward with xh = (x - mean) rstd, a = dout (1 + scale) gamma:
//   dx = dres + rstd (a - mean_c(a) - xh mean_c(a xh));  per (b, c): S0 = sum_hw dout, S1 = sum_hw dout xh
//   dshift = S0, dscale = gamma S1 + beta S0, dgamma = sum_b (1 + scale) S1, dbeta = sum_b (1 + scale) S0   (al_finish_kernel)
//
// Deterministic: a workgroup owns a contiguous pixel range of one slice whose length depends on hw only; a lane keeps its own
// channels across the pixels it visits, the row slots are combined in LDS in slot order, the workgroups' partials go to the
// workspace and are summed in order (launch_sum); dgamma and dbeta add the slices in index order.  No atomics.  Every per-slice
// result is the same bits alone or in a batch.  C % 64 == 0, C <= 512.
#include "fd_train_common.h"

namespace {

constexpr int AL_G = 16;                   // partials per first-level sum
constexpr int AL_FROWS = 64;               // pixels per workgroup of the two forwards

struct AlPlan {
    int lpr, vpl, rpb, ch, nchunk, M1;
};

bool al_shape_ok(int B, int64_t hw, int C) { return B > 0 && B < 65536 && hw > 0 && hw < (1ll << 31) && C > 0 && C % 64 == 0 && C <= 512; }

AlPlan al_plan(int64_t hw, int C) {
    AlPlan p;
    p.lpr = C / 4 <= 16 ? 16 : (C / 4 <= 32 ? 32 : 64);
    p.vpl = (C + 4 * p.lpr - 1) / (4 * p.lpr);                           // 1 or 2 for C <= 512
    p.rpb = 256 / p.lpr;
    // pixels per workgroup of the backwards: ~512 workgroups from one slice, 16 .. 512 pixels each (a function of hw alone)
    const int64_t ch = ((hw + 511) / 512 + 15) / 16 * 16;
    p.ch = (int)(ch < 16 ? 16 : (ch > 512 ? 512 : ch));
    p.nchunk = (int)((hw + p.ch - 1) / p.ch);
    // M1 first-level sums per slice are what one thread per channel of al_finish_kernel (and of the second launch_sum) adds
    // serially: <= 32 while hw <= 512 * 512, where ch reaches its cap; beyond that M1 = hw / 8192 grows with hw (4 x the
    // training resolution: 128 steps per slice), which a third level of sums would bound if such sizes came up
    p.M1 = (p.nchunk + AL_G - 1) / AL_G;
    return p;
}

// workspace of a backward with nq sums per (b, c): the workgroups' partials, then the first-level sums
int64_t al_ws_floats(int B, const AlPlan &p, int nq, int C) {
    return round4((int64_t)B * p.nchunk * nq * C) + round4((int64_t)B * p.M1 * nq * C);
}

__device__ __forceinline__ float al_group_sum(float t, int lpr) {
    for (int o = 1; o < lpr; o <<= 1) t += __shfl_xor(t, o, 64);
    return t;
}

__device__ __forceinline__ float al_sum4(const f32x4 &v) { return (v[0] + v[1]) + (v[2] + v[3]); }

__device__ __forceinline__ float al_dot4(const f32x4 &a, const f32x4 &b) { return (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]); }

// this lane's vectors of a per-channel row p (NULL: fill), channels past C filled too
template <int VPL>
__device__ __forceinline__ void al_load_row(const float *__restrict__ p, int C, int lpr, int sub, float fill, f32x4 (&v)[VPL]) {
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int c = (j * lpr + sub) * 4;
        v[j] = f32x4{fill, fill, fill, fill};
        if (p && c < C) v[j] = *(const f32x4 *)(p + c);
    }
}

// the row slots' column sums in slot order -> pp[NQ][C]; red holds NQ 1024 VPL floats
template <int VPL, int NQ>
__device__ __forceinline__ void al_col_sums(float *__restrict__ red, const f32x4 (&acc)[NQ][VPL], float *__restrict__ pp, int C, int lpr) {
    const int tid = threadIdx.x, sub = tid % lpr, slot = tid / lpr, rpb = 256 / lpr, cw = lpr * 4 * VPL;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int j = 0; j < VPL; ++j) *(f32x4 *)(red + (slot * NQ + q) * cw + (j * lpr + sub) * 4) = acc[q][j];
    __syncthreads();
    for (int idx = tid; idx < NQ * C; idx += 256) {
        const int which = idx / C, c = idx - which * C;
        float v = 0.f;
        for (int sl = 0; sl < rpb; ++sl) v += red[(sl * NQ + which) * cw + c];
        pp[idx] = v;
    }
}

// grid (pixel block of AL_FROWS, b)
template <int VPL>
__global__ __launch_bounds__(256) void al_fwd_kernel(const float *__restrict__ x, const float *__restrict__ gamma,
                                                    const float *__restrict__ beta, float eps, const float *__restrict__ shift,
                                                    const float *__restrict__ scale, int ld_mod, float *__restrict__ out,
                                                    float *__restrict__ stats, int64_t hw, int C, int lpr) {
    const int tid = threadIdx.x, sub = tid % lpr, slot = tid / lpr, rpb = 256 / lpr;
    const int64_t b = blockIdx.y;
    const int64_t r0 = (int64_t)blockIdx.x * AL_FROWS;
    const float invC = 1.0f / (float)C;
    f32x4 gm[VPL], bt[VPL], sc[VPL], sh[VPL];
    al_load_row<VPL>(gamma, C, lpr, sub, 1.f, gm);
    al_load_row<VPL>(beta, C, lpr, sub, 0.f, bt);
    al_load_row<VPL>(scale + b * ld_mod, C, lpr, sub, 0.f, sc);
    al_load_row<VPL>(shift + b * ld_mod, C, lpr, sub, 0.f, sh);
#pragma unroll
    for (int j = 0; j < VPL; ++j) sc[j] += 1.0f;
    for (int rr = slot; rr < AL_FROWS; rr += rpb) {
        const bool active = r0 + rr < hw;                                // a whole lane group at once
        const int64_t row = b * hw + (active ? r0 + rr : 0);
        f32x4 v[VPL];
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const int c = (j * lpr + sub) * 4;
            v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (c < C) v[j] = *(const f32x4 *)(x + row * C + c);
            s += al_sum4(v[j]);
        }
        const float mean = al_group_sum(s, lpr) * invC;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const int c = (j * lpr + sub) * 4;
            if (c < C) {
                v[j] -= mean;
                q += al_dot4(v[j], v[j]);
            }
        }
        const float rstd = rsqrtf(al_group_sum(q, lpr) * invC + eps);
        if (!active) continue;
        if (sub == 0) {
            stats[2 * row] = mean;
            stats[2 * row + 1] = rstd;
        }
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const int c = (j * lpr + sub) * 4;
            if (c >= C) continue;
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (v[j][e] * rstd * gm[j][e] + bt[j][e]) * sc[j][e] + sh[j][e];
            *(f32x4 *)(out + row * C + c) = o;
        }
    }
}

// grid (chunk, b): pixels [chunk ch, +ch) of slice b, rpb at a time; part[b][chunk][S0 C | S1 C]
template <int VPL>
__global__ __launch_bounds__(256) void al_bwd_kernel(const float *__restrict__ dout, const float *__restrict__ x,
                                                    const float *__restrict__ stats, const float *__restrict__ gamma,
                                                    const float *__restrict__ scale, int ld_mod, const float *__restrict__ dres,
                                                    float *__restrict__ dx, float *__restrict__ part, int64_t hw, int C, int lpr,
                                                    int ch) {
    __shared__ __attribute__((aligned(16))) float red[2 * 1024 * VPL];
    const int tid = threadIdx.x, sub = tid % lpr, slot = tid / lpr, rpb = 256 / lpr;
    const int64_t b = blockIdx.y;
    const int64_t r0 = (int64_t)blockIdx.x * ch;
    const float invC = 1.0f / (float)C;
    f32x4 sg[VPL], sc[VPL], acc[2][VPL];
    al_load_row<VPL>(gamma, C, lpr, sub, 1.f, sg);
    al_load_row<VPL>(scale + b * ld_mod, C, lpr, sub, 0.f, sc);
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        sg[j] *= 1.0f + sc[j];                                           // a = dout (1 + scale) gamma
        acc[0][j] = acc[1][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int rr = slot; rr < ch; rr += rpb) {
        const bool active = r0 + rr < hw;
        const int64_t row = b * hw + (active ? r0 + rr : 0);
        const float mean = stats[2 * row], rstd = stats[2 * row + 1];
        f32x4 xh[VPL], a[VPL];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const int c = (j * lpr + sub) * 4;
            xh[j] = a[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (c < C && active) {
                const f32x4 xv = *(const f32x4 *)(x + row * C + c);
                const f32x4 g = *(const f32x4 *)(dout + row * C + c);
                xh[j] = (xv - mean) * rstd;
                a[j] = g * sg[j];
                acc[0][j] += g;
                acc[1][j] += g * xh[j];
                s1 += al_sum4(a[j]);
                s2 += al_dot4(a[j], xh[j]);
            }
        }
        s1 = al_group_sum(s1, lpr) * invC;
        s2 = al_group_sum(s2, lpr) * invC;
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const int c = (j * lpr + sub) * 4;
            if (c < C && active) {
                f32x4 o = rstd * (a[j] - s1 - xh[j] * s2);
                if (dres) o += *(const f32x4 *)(dres + row * C + c);
                *(f32x4 *)(dx + row * C + c) = o;
            }
        }
    }
    al_col_sums<VPL, 2>(red, acc, part + (b * gridDim.x + blockIdx.x) * 2 * C, C, lpr);
}

// stage [B][M1][S0 C | S1 C] summed over M1 in order -> dshift, dscale [B][ld_dmod]; dgamma, dbeta [C] over b in order (or NULL)
__global__ __launch_bounds__(256) void al_finish_kernel(const float *__restrict__ stage, int M1, int B, int C, const float *__restrict__ gamma,
                                                       const float *__restrict__ beta, const float *__restrict__ scale, int ld_mod,
                                                       float *__restrict__ dshift, float *__restrict__ dscale, int ld_dmod,
                                                       float *__restrict__ dgamma, float *__restrict__ dbeta) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float g = gamma ? gamma[c] : 1.0f, bt = beta ? beta[c] : 0.0f;
    float dg = 0.f, db = 0.f;
    for (int b = 0; b < B; ++b) {
        const float *sp = stage + (int64_t)b * M1 * 2 * C + c;
        float S0 = 0.f, S1 = 0.f;
        for (int m = 0; m < M1; ++m) {
            S0 += sp[(int64_t)m * 2 * C];
            S1 += sp[(int64_t)m * 2 * C + C];
        }
        const float sc1 = 1.0f + scale[(int64_t)b * ld_mod + c];
        dshift[(int64_t)b * ld_dmod + c] = S0;
        dscale[(int64_t)b * ld_dmod + c] = g * S1 + bt * S0;
        dg += sc1 * S1;
        db += sc1 * S0;
    }
    if (dgamma) {
        dgamma[c] = dg;
        dbeta[c] = db;
    }
}

// grid (pixel block of AL_FROWS, b)
template <int VPL>
__global__ __launch_bounds__(256) void gr_fwd_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                    const float *__restrict__ gate, int ld_mod, float *__restrict__ out, int64_t hw,
                                                    int C, int lpr) {
    const int tid = threadIdx.x, sub = tid % lpr, slot = tid / lpr, rpb = 256 / lpr;
    const int64_t b = blockIdx.y;
    const int64_t r0 = (int64_t)blockIdx.x * AL_FROWS;
    f32x4 gt[VPL];
    al_load_row<VPL>(gate + b * ld_mod, C, lpr, sub, 0.f, gt);
    for (int rr = slot; rr < AL_FROWS && r0 + rr < hw; rr += rpb) {
        const int64_t row = b * hw + r0 + rr;
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const int c = (j * lpr + sub) * 4;
            if (c >= C) continue;
            const f32x4 xv = *(const f32x4 *)(x + row * C + c), yv = *(const f32x4 *)(y + row * C + c);
            *(f32x4 *)(out + row * C + c) = xv + gt[j] * yv;
        }
    }
}

// grid (chunk, b): part[b][chunk][C] = the chunk's sum of dout y
template <int VPL>
__global__ __launch_bounds__(256) void gr_bwd_kernel(const float *__restrict__ dout, const float *__restrict__ y,
                                                    const float *__restrict__ gate, int ld_mod, float *__restrict__ dy,
                                                    float *__restrict__ part, int64_t hw, int C, int lpr, int ch) {
    __shared__ __attribute__((aligned(16))) float red[1024 * VPL];
    const int tid = threadIdx.x, sub = tid % lpr, slot = tid / lpr, rpb = 256 / lpr;
    const int64_t b = blockIdx.y;
    const int64_t r0 = (int64_t)blockIdx.x * ch;
    f32x4 gt[VPL], acc[1][VPL];
    al_load_row<VPL>(gate + b * ld_mod, C, lpr, sub, 0.f, gt);
#pragma unroll
    for (int j = 0; j < VPL; ++j) acc[0][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int rr = slot; rr < ch && r0 + rr < hw; rr += rpb) {
        const int64_t row = b * hw + r0 + rr;
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const int c = (j * lpr + sub) * 4;
            if (c >= C) continue;
            const f32x4 g = *(const f32x4 *)(dout + row * C + c), yv = *(const f32x4 *)(y + row * C + c);
            acc[0][j] += g * yv;
            *(f32x4 *)(dy + row * C + c) = gt[j] * g;
        }
    }
    al_col_sums<VPL, 1>(red, acc, part + (b * gridDim.x + blockIdx.x) * C, C, lpr);
}

bool al_mod_ok(const float *p, int ld, int C) { return al16(p) && ld % 4 == 0 && ld >= C; }

}  // namespace

#define FD_AL_VPL(KERNEL, ...)                                                                       \
    do {                                                                                             \
        if (p.vpl == 1) hipLaunchKernelGGL(KERNEL<1>, __VA_ARGS__);                                  \
        else hipLaunchKernelGGL(KERNEL<2>, __VA_ARGS__);                                             \
    } while (0)

extern "C" int fd_adaln_fwd_f32(const float *x, const float *gamma, const float *beta, float eps, const float *shift,
                                const float *scale, int ld_mod, float *out, float *stats, int B, int64_t hw, int C, void *stream) {
    FD_REQUIRE(x && shift && scale && out && stats, "fd_adaln_fwd_f32: null pointer");
    FD_REQUIRE((gamma == nullptr) == (beta == nullptr), "fd_adaln_fwd_f32: gamma and beta must both be set or both be NULL");
    FD_REQUIRE(al_shape_ok(B, hw, C), "fd_adaln_fwd_f32: unsupported shape B=%d hw=%lld C=%d (C %% 64 == 0, C <= 512)", B,
               (long long)hw, C);
    FD_REQUIRE(al_mod_ok(shift, ld_mod, C) && al_mod_ok(scale, ld_mod, C),
               "fd_adaln_fwd_f32: shift / scale must be 16-byte aligned with a row stride that is a multiple of 4 and >= C (ld_mod=%d)",
               ld_mod);
    FD_REQUIRE(al16(x) && al16(gamma) && al16(beta) && al16(out), "fd_adaln_fwd_f32: tensors must be 16-byte aligned");
    const AlPlan p = al_plan(hw, C);
    FD_AL_VPL(al_fwd_kernel, dim3((unsigned)((hw + AL_FROWS - 1) / AL_FROWS), (unsigned)B), dim3(256), 0, (hipStream_t)stream, x, gamma,
              beta, eps, shift, scale, ld_mod, out, stats, hw, C, p.lpr);
    FD_LAUNCH_OK("fd_adaln_fwd_f32");
    return FD_OK;
}

extern "C" int64_t fd_adaln_bwd_ws_floats(int B, int64_t hw, int C) {
    if (!al_shape_ok(B, hw, C)) return 0;
    return al_ws_floats(B, al_plan(hw, C), 2, C);
}

extern "C" int fd_adaln_bwd_f32(const float *dout, const float *x, const float *stats, const float *gamma, const float *beta,
                                const float *scale, int ld_mod, const float *dres, float *dx, float *dshift, float *dscale,
                                int ld_dmod, float *dgamma, float *dbeta, float *ws, int B, int64_t hw, int C, void *stream) {
    FD_REQUIRE(dout && x && stats && scale && dx && dshift && dscale && ws, "fd_adaln_bwd_f32: null pointer");
    FD_REQUIRE((gamma == nullptr) == (beta == nullptr) && (gamma == nullptr) == (dgamma == nullptr) &&
                   (gamma == nullptr) == (dbeta == nullptr),
               "fd_adaln_bwd_f32: gamma, beta, dgamma and dbeta must all be set or all be NULL");
    FD_REQUIRE(al_shape_ok(B, hw, C), "fd_adaln_bwd_f32: unsupported shape B=%d hw=%lld C=%d (C %% 64 == 0, C <= 512)", B,
               (long long)hw, C);
    FD_REQUIRE(al_mod_ok(scale, ld_mod, C) && ld_dmod >= C,
               "fd_adaln_bwd_f32: scale must be 16-byte aligned with a row stride that is a multiple of 4 and >= C, ld_dmod >= C "
               "(ld_mod=%d ld_dmod=%d)", ld_mod, ld_dmod);
    FD_REQUIRE(al16(dout) && al16(x) && al16(gamma) && al16(dres) && al16(dx) && al16(ws),
               "fd_adaln_bwd_f32: tensors must be 16-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    const AlPlan p = al_plan(hw, C);
    const int64_t Q = 2 * (int64_t)C;
    float *part = ws, *stage = part + round4((int64_t)B * p.nchunk * Q);
    FD_AL_VPL(al_bwd_kernel, dim3((unsigned)p.nchunk, (unsigned)B), dim3(256), 0, st, dout, x, stats, gamma, scale, ld_mod, dres, dx,
              part, hw, C, p.lpr, p.ch);
    launch_sum(part, Q, (int64_t)p.nchunk * Q, p.nchunk, (int)Q, AL_G, stage, Q, (int64_t)p.M1 * Q, B, st);
    hipLaunchKernelGGL(al_finish_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, stage, p.M1, B, C, gamma, beta, scale,
                       ld_mod, dshift, dscale, ld_dmod, dgamma, dbeta);
    FD_LAUNCH_OK("fd_adaln_bwd_f32");
    return FD_OK;
}

extern "C" int fd_gate_res_fwd_f32(const float *x, const float *y, const float *gate, int ld_mod, float *out, int B, int64_t hw,
                                   int C, void *stream) {
    FD_REQUIRE(x && y && gate && out, "fd_gate_res_fwd_f32: null pointer");
    FD_REQUIRE(al_shape_ok(B, hw, C), "fd_gate_res_fwd_f32: unsupported shape B=%d hw=%lld C=%d (C %% 64 == 0, C <= 512)", B,
               (long long)hw, C);
    FD_REQUIRE(al_mod_ok(gate, ld_mod, C),
               "fd_gate_res_fwd_f32: gate must be 16-byte aligned with a row stride that is a multiple of 4 and >= C (ld_mod=%d)", ld_mod);
    FD_REQUIRE(al16(x) && al16(y) && al16(out), "fd_gate_res_fwd_f32: tensors must be 16-byte aligned");
    const AlPlan p = al_plan(hw, C);
    FD_AL_VPL(gr_fwd_kernel, dim3((unsigned)((hw + AL_FROWS - 1) / AL_FROWS), (unsigned)B), dim3(256), 0, (hipStream_t)stream, x, y,
              gate, ld_mod, out, hw, C, p.lpr);
    FD_LAUNCH_OK("fd_gate_res_fwd_f32");
    return FD_OK;
}

extern "C" int64_t fd_gate_res_bwd_ws_floats(int B, int64_t hw, int C) {
    if (!al_shape_ok(B, hw, C)) return 0;
    return al_ws_floats(B, al_plan(hw, C), 1, C);
}

extern "C" int fd_gate_res_bwd_f32(const float *dout, const float *y, const float *gate, int ld_mod, float *dy, float *dgate,
                                   int ld_dmod, float *ws, int B, int64_t hw, int C, void *stream) {
    FD_REQUIRE(dout && y && gate && dy && dgate && ws, "fd_gate_res_bwd_f32: null pointer");
    FD_REQUIRE(al_shape_ok(B, hw, C), "fd_gate_res_bwd_f32: unsupported shape B=%d hw=%lld C=%d (C %% 64 == 0, C <= 512)", B,
               (long long)hw, C);
    FD_REQUIRE(al_mod_ok(gate, ld_mod, C) && ld_dmod >= C,
               "fd_gate_res_bwd_f32: gate must be 16-byte aligned with a row stride that is a multiple of 4 and >= C, ld_dmod >= C "
               "(ld_mod=%d ld_dmod=%d)", ld_mod, ld_dmod);
    FD_REQUIRE(al16(dout) && al16(y) && al16(dy) && al16(ws), "fd_gate_res_bwd_f32: tensors must be 16-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    const AlPlan p = al_plan(hw, C);
    float *part = ws, *stage = part + round4((int64_t)B * p.nchunk * C);
    FD_AL_VPL(gr_bwd_kernel, dim3((unsigned)p.nchunk, (unsigned)B), dim3(256), 0, st, dout, y, gate, ld_mod, dy, part, hw, C, p.lpr,
              p.ch);
    launch_sum(part, C, (int64_t)p.nchunk * C, p.nchunk, C, AL_G, stage, C, (int64_t)p.M1 * C, B, st);
    launch_sum(stage, C, (int64_t)p.M1 * C, p.M1, C, p.M1, dgate, 0, ld_dmod, B, st);
    FD_LAUNCH_OK("fd_gate_res_bwd_f32");
    return FD_OK;
}
#undef FD_AL_VPL
