// fd_train_step.hip -- what lies between a batch and the U-Net, and between the gradients and the next weights, of one training
// step of the reference (src/DADiff.py:1382-1499 ResidualDiffusion.forward / q_sample / p_losses, 1689-1725 Trainer.train):
//
//   fd_res_qsample_f32     normalize + x_res + q_sample + the cat + the two time inputs, one launch
//   fd_res_loss_f32        l1 / l2 loss (per-slice mean, batch mean, times a scale) and its gradient, one pass + two small sums
//   fd_scale_dev_f32       that gradient times the scalar autograd hands back, read from device memory
//   fd_opt_sumsq_f32       per chunk sum of g^2                                  \  clip_grad_norm_(max_norm) + Adam + zero_grad
//   fd_opt_clip_coef       total norm, clip coefficient, non-finite flag, steps   > + the EMA update, over a chunk table the host
//   fd_opt_adam_ema_f32    the update itself                                     /  builds once
//   fd_opt_radam_ema_f32   the same with torch.optim.RAdam's update rule (two U-Nets, src/DADiff.py:1598-1602) in Adam's place
//
// No float atomics; every sum has a fixed order that depends on the tensor's own size only (a slice's loss partials on npix, a
// parameter's chunks on its numel); nothing synchronises with the host; the clip coefficient, the non-finite flag and the Adam step
// counts live in device memory.  Every lane owns the same elements on the 16-byte path and on the scalar path, and the arithmetic is
// written with explicit fmaf, so the two paths give the same bits.
#include <cfloat>
#include "fd_train_common.h"
#include "fd_keyed_noise.h"

namespace {

constexpr int OPT_CHUNK = 4096;        // elements of a parameter per workgroup: 256 lanes x 4 vectors of 4
constexpr int OPT_VPL = OPT_CHUNK / 1024;
constexpr int LS_CHUNK = 8192;         // pixels of a slice per workgroup of the loss: 256 lanes x 8 vectors of 4
constexpr int LS_VPL = LS_CHUNK / 1024;
constexpr int LS_G = 32;               // partials per launch_sum group
constexpr int TT_COLS = 8;             // per-tensor table row: p, g, m, v, ema, flags, 0, 0 (int64 each)
constexpr int64_t TT_ACTIVE = 1, TT_VEC = 2;

// ---- q_sample ------------------------------------------------------------------------------------------------------------------
// grid (groups of four pixels / 256, b); one group per lane.  VEC: npix % 4 == 0 and every pointer 16-byte aligned.
template <bool VEC, bool KEYED>
__global__ __launch_bounds__(256) void qsample_kernel(const float *__restrict__ x_start, const float *__restrict__ x_input,
                                                     const int64_t *__restrict__ t, const float *__restrict__ acs,
                                                     const float *__restrict__ bcs, int T, const float *__restrict__ noise,
                                                     const int64_t *__restrict__ seeds, int noise_step, int normalize,
                                                     float *__restrict__ x_in, float *__restrict__ x_res,
                                                     float *__restrict__ noise_out, float *__restrict__ times, int B, int64_t npix) {
    const int b = blockIdx.y;
    const int64_t tb = min(max(t[b], (int64_t)0), (int64_t)T - 1);       // a timestep outside the table reads its nearest row
    const float ac = acs[tb], bc = bcs[tb];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        times[b] = ac * (float)T;
        times[B + b] = bc * (float)T;
    }
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i0 = 4 * g;
    if (i0 >= npix) return;
    const int n = (int)min((int64_t)4, npix - i0);
    const int64_t row = (int64_t)b * npix + i0;
    float x0[4], xi[4], z[4], xt[4], xr[4];
    load4<VEC>(x_start + row, n, x0);
    load4<VEC>(x_input + row, n, xi);
    if (KEYED) keyed_normal4((uint64_t)seeds[b], (uint32_t)noise_step, (uint32_t)g, z);
    else load4<VEC>(noise + row, n, z);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (normalize) {
            x0[e] = fmaf(2.f, x0[e], -1.f);
            xi[e] = fmaf(2.f, xi[e], -1.f);
        }
        xr[e] = xi[e] - x0[e];
        xt[e] = fmaf(bc, z[e], fmaf(ac, xr[e], x0[e]));
    }
    store4<VEC>(x_in + (int64_t)b * 2 * npix + i0, n, xt);
    store4<VEC>(x_in + ((int64_t)b * 2 + 1) * npix + i0, n, xi);
    store4<VEC>(x_res + row, n, xr);
    if (KEYED) store4<VEC>(noise_out + row, n, z);
}

// ---- loss ----------------------------------------------------------------------------------------------------------------------
// grid (chunk of LS_CHUNK pixels, b): part[b][chunk] = the chunk's sum of |d| or d^2, dpred = c sign(d) or c d
template <bool VEC, bool L2>
__global__ __launch_bounds__(256) void loss_kernel(const float *__restrict__ pred, const float *__restrict__ target,
                                                  float *__restrict__ dpred, float *__restrict__ part, int64_t npix, float c) {
    __shared__ float red[256];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int64_t base = (int64_t)b * npix, c0 = (int64_t)blockIdx.x * LS_CHUNK;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < LS_VPL; ++j) {
        const int64_t i0 = c0 + 4 * (j * 256 + tid);
        if (i0 >= npix) continue;
        const int n = (int)min((int64_t)4, npix - i0);
        float p[4], q[4], d[4];
        load4<VEC>(pred + base + i0, n, p);
        load4<VEC>(target + base + i0, n, q);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float df = p[e] - q[e];                                // 0 - 0 past the end
            acc = L2 ? fmaf(df, df, acc) : acc + fabsf(df);
            d[e] = L2 ? c * df : (df > 0.f ? c : (df < 0.f ? -c : df));  // sign(0) = 0, a NaN stays one
        }
        store4<VEC>(dpred + base + i0, n, d);
    }
    const float s = block_sum256(acc, red);
    if (tid == 0) part[(int64_t)b * gridDim.x + blockIdx.x] = s;
}

// one workgroup: loss = scale_over_b * sum_b (sum_m stage[b][m]) * inv_npix, in double, slices in order
__global__ __launch_bounds__(256) void loss_finish_kernel(const float *__restrict__ stage, int M, int B, double inv_npix,
                                                         double scale_over_b, float *__restrict__ loss) {
    __shared__ double sd[256];
    const int tid = threadIdx.x;
    double tot = 0.0;
    for (int b = tid; b < B; b += 256) {
        double s = 0.0;
        for (int m = 0; m < M; ++m) s += (double)stage[(int64_t)b * M + m];
        tot += s * inv_npix;
    }
    sd[tid] = tot;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < 256 && i < B; ++i) s += sd[i];
        loss[0] = (float)(s * scale_over_b);
    }
}

// out = s[0] x: the loss gradient times the scalar that autograd hands back, read on the device
template <bool VEC>
__global__ __launch_bounds__(256) void scale_dev_kernel(const float *__restrict__ x, const float *__restrict__ s,
                                                       float *__restrict__ out, int64_t n) {
    const int64_t i0 = 4 * ((int64_t)blockIdx.x * 256 + threadIdx.x);
    if (i0 >= n) return;
    const int m = (int)min((int64_t)4, n - i0);
    const float k = s[0];
    float v[4];
    if (VEC && m == 4) load4<true>(x + i0, 4, v);
    else load4<false>(x + i0, m, v);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] *= k;
    if (VEC && m == 4) store4<true>(out + i0, 4, v);
    else store4<false>(out + i0, m, v);
}

int ls_nchunk(int64_t npix) { return (int)((npix + LS_CHUNK - 1) / LS_CHUNK); }

// ---- the optimiser -------------------------------------------------------------------------------------------------------------
struct OptChunk {
    const int64_t *row;
    int64_t off;
    int len;
    bool active, vec;
};

__device__ __forceinline__ OptChunk opt_chunk(const int64_t *__restrict__ chunks, const int64_t *__restrict__ tensors) {
    const int64_t *c = chunks + 3 * (int64_t)blockIdx.x;
    OptChunk o;
    o.row = tensors + TT_COLS * c[0];
    o.off = c[1];
    o.len = (int)c[2];
    o.active = (o.row[5] & TT_ACTIVE) != 0;
    o.vec = (o.row[5] & TT_VEC) != 0;
    return o;
}

// grid (chunk): part[chunk] = the chunk's sum of g^2, 0 for a tensor without a gradient
__global__ __launch_bounds__(256) void opt_sumsq_kernel(const int64_t *__restrict__ chunks, const int64_t *__restrict__ tensors,
                                                       float *__restrict__ part) {
    __shared__ float red[256];
    const int tid = threadIdx.x;
    const OptChunk o = opt_chunk(chunks, tensors);
    if (!o.active) {
        if (tid == 0) part[blockIdx.x] = 0.f;
        return;
    }
    const float *g = (const float *)o.row[1] + o.off;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < OPT_VPL; ++j) {
        const int i0 = 4 * (j * 256 + tid);
        if (i0 >= o.len) continue;
        const int n = min(4, o.len - i0);
        float v[4];
        if (o.vec && n == 4) load4<true>(g + i0, 4, v);
        else load4<false>(g + i0, n, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = fmaf(v[e], v[e], acc);
    }
    const float s = block_sum256(acc, red);
    if (tid == 0) part[blockIdx.x] = s;
}

// one workgroup.  Lane i adds partials [i seg, (i + 1) seg) in index order in double, lane 0 adds the 256 sums in order:
// rec = {total_norm, coef, nonfinite, 0}; then the step count of every tensor with a gradient goes up by one, unless the step is skipped
__global__ __launch_bounds__(256) void opt_clip_kernel(const float *__restrict__ part, int nchunk, const int64_t *__restrict__ tensors,
                                                      int *__restrict__ steps, int nt, float max_norm, int skip_nonfinite,
                                                      float *__restrict__ rec) {
    __shared__ double sd[256];
    __shared__ int s_skip;
    const int tid = threadIdx.x;
    const int seg = (nchunk + 255) / 256;
    const int i1 = min(nchunk, (tid + 1) * seg);
    double s = 0.0;
    for (int i = tid * seg; i < i1; ++i) s += (double)part[i];
    sd[tid] = s;
    __syncthreads();
    if (tid == 0) {
        double tot = 0.0;
        for (int i = 0; i < 256; ++i) tot += sd[i];
        const float norm = (float)sqrt(tot);
        const bool bad = !(fabsf(norm) <= FLT_MAX);
        float coef = 1.f;
        if (max_norm >= 0.f) {                                           // clip_grad_norm_'s arithmetic; a NaN stays one
            const float c = max_norm / (norm + 1e-6f);
            coef = c > 1.f ? 1.f : c;
        }
        rec[0] = norm;
        rec[1] = coef;
        rec[2] = bad ? 1.f : 0.f;
        rec[3] = 0.f;
        s_skip = bad && skip_nonfinite;
    }
    __syncthreads();
    if (s_skip) return;
    for (int i = tid; i < nt; i += 256)
        if (tensors[(int64_t)TT_COLS * i + 5] & TT_ACTIVE) steps[i] += 1;
}

struct AdamK {
    float coef, w1, beta2, w2, step_size, bc2_sqrt, eps, ema_w;
    int ema_mode, zero_grad;
};

// RULE of adam4: Adam; RAdam on a rectified step (step_size holds lr / bc1 * r * sqrt(bc2), eps joins sqrt(v) uncorrected);
// RAdam before that (step_size = lr / bc1, v is updated and does not enter p)
constexpr int RULE_ADAM = 0, RULE_RADAM_RECT = 1, RULE_RADAM_PLAIN = 2;

template <bool VEC, int RULE = RULE_ADAM>
__device__ __forceinline__ void adam4(const AdamK &k, float *p, float *g, float *m, float *v, float *ema, int n) {
    float pv[4], gv[4], mv[4], vv[4], ev[4];
    load4<VEC>(p, n, pv);
    load4<VEC>(g, n, gv);
    load4<VEC>(m, n, mv);
    load4<VEC>(v, n, vv);
    const bool lerp = ema && k.ema_mode == 2;
    if (lerp) load4<VEC>(ema, n, ev);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float gc = k.coef * gv[e];
        mv[e] = fmaf(k.w1, gc - mv[e], mv[e]);
        vv[e] = fmaf(k.w2 * gc, gc, k.beta2 * vv[e]);
        if constexpr (RULE == RULE_ADAM) {
            const float denom = sqrtf(vv[e]) / k.bc2_sqrt + k.eps;
            pv[e] = fmaf(-k.step_size, mv[e] / denom, pv[e]);
        } else if constexpr (RULE == RULE_RADAM_RECT) {
            pv[e] = fmaf(-k.step_size, mv[e] / (sqrtf(vv[e]) + k.eps), pv[e]);
        } else {
            pv[e] = fmaf(-k.step_size, mv[e], pv[e]);
        }
        if (lerp) ev[e] = fmaf(-k.ema_w, ev[e] - pv[e], ev[e]);
        gv[e] = 0.f;
    }
    store4<VEC>(p, n, pv);
    store4<VEC>(m, n, mv);
    store4<VEC>(v, n, vv);
    if (k.zero_grad) store4<VEC>(g, n, gv);
    if (ema && k.ema_mode == 1) store4<VEC>(ema, n, pv);
    if (lerp) store4<VEC>(ema, n, ev);
}

// grid (chunk)
__global__ __launch_bounds__(256) void opt_adam_kernel(const int64_t *__restrict__ chunks, const int64_t *__restrict__ tensors,
                                                      const int *__restrict__ steps, const float *__restrict__ rec, double lr,
                                                      double beta1, double beta2, double eps, int ema_mode, double ema_decay,
                                                      int zero_grad, int skip_nonfinite) {
    __shared__ float s_bc[2];
    const int tid = threadIdx.x;
    const OptChunk o = opt_chunk(chunks, tensors);
    if (!o.active) return;
    if (skip_nonfinite && rec[2] != 0.f) return;
    if (tid == 0) {                                                      // Adam's bias corrections of this tensor's step, in double
        const double step = (double)steps[chunks[3 * (int64_t)blockIdx.x]];
        const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
        s_bc[0] = (float)(lr / bc1);
        s_bc[1] = (float)sqrt(bc2);
    }
    __syncthreads();
    AdamK k;
    k.coef = rec[1];
    k.w1 = (float)(1.0 - beta1);
    k.beta2 = (float)beta2;
    k.w2 = (float)(1.0 - beta2);
    k.step_size = s_bc[0];
    k.bc2_sqrt = s_bc[1];
    k.eps = (float)eps;
    k.ema_w = (float)(1.0 - ema_decay);
    k.ema_mode = ema_mode;
    k.zero_grad = zero_grad;
    float *p = (float *)o.row[0] + o.off, *g = (float *)o.row[1] + o.off, *m = (float *)o.row[2] + o.off;
    float *v = (float *)o.row[3] + o.off, *ema = o.row[4] ? (float *)o.row[4] + o.off : nullptr;
#pragma unroll
    for (int j = 0; j < OPT_VPL; ++j) {
        const int i0 = 4 * (j * 256 + tid);
        if (i0 >= o.len) continue;
        const int n = min(4, o.len - i0);
        if (o.vec && n == 4) adam4<true>(k, p + i0, g + i0, m + i0, v + i0, ema ? ema + i0 : nullptr, 4);
        else adam4<false>(k, p + i0, g + i0, m + i0, v + i0, ema ? ema + i0 : nullptr, n);
    }
}

template <int RULE>
__device__ __forceinline__ void radam_chunk(const AdamK &k, const OptChunk &o, int tid) {
    float *p = (float *)o.row[0] + o.off, *g = (float *)o.row[1] + o.off, *m = (float *)o.row[2] + o.off;
    float *v = (float *)o.row[3] + o.off, *ema = o.row[4] ? (float *)o.row[4] + o.off : nullptr;
#pragma unroll
    for (int j = 0; j < OPT_VPL; ++j) {
        const int i0 = 4 * (j * 256 + tid);
        if (i0 >= o.len) continue;
        const int n = min(4, o.len - i0);
        if (o.vec && n == 4) adam4<true, RULE>(k, p + i0, g + i0, m + i0, v + i0, ema ? ema + i0 : nullptr, 4);
        else adam4<false, RULE>(k, p + i0, g + i0, m + i0, v + i0, ema ? ema + i0 : nullptr, n);
    }
}

// grid (chunk).  torch.optim.RAdam's update (_single_tensor_radam) of this chunk's tensor at its own step count: the variance
// rectification is on or off per tensor, so per workgroup, and tensors at different steps take different branches in one launch
__global__ __launch_bounds__(256) void opt_radam_kernel(const int64_t *__restrict__ chunks, const int64_t *__restrict__ tensors,
                                                       const int *__restrict__ steps, const float *__restrict__ rec, double lr,
                                                       double beta1, double beta2, double eps, int ema_mode, double ema_decay,
                                                       int zero_grad, int skip_nonfinite) {
    __shared__ float s_step;
    __shared__ int s_rect;
    const int tid = threadIdx.x;
    const OptChunk o = opt_chunk(chunks, tensors);
    if (!o.active) return;
    if (skip_nonfinite && rec[2] != 0.f) return;
    if (tid == 0) {                                                      // this tensor's scalars, in double (radam_scalars)
        const double step = (double)steps[chunks[3 * (int64_t)blockIdx.x]];
        const double b2s = pow(beta2, step);
        const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - b2s;
        const double rho_inf = 2.0 / (1.0 - beta2) - 1.0, rho = rho_inf - 2.0 * step * b2s / bc2;
        double size = lr / bc1;
        const int rect = rho > 5.0;                                      // rho <= rho_inf: with rho_inf <= 5 nothing divides by rho_inf - 4
        if (rect) size *= sqrt((rho - 4.0) * (rho - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho)) * sqrt(bc2);
        s_step = (float)size;
        s_rect = rect;
    }
    __syncthreads();
    AdamK k;
    k.coef = rec[1];
    k.w1 = (float)(1.0 - beta1);
    k.beta2 = (float)beta2;
    k.w2 = (float)(1.0 - beta2);
    k.step_size = s_step;
    k.bc2_sqrt = 1.f;
    k.eps = (float)eps;
    k.ema_w = (float)(1.0 - ema_decay);
    k.ema_mode = ema_mode;
    k.zero_grad = zero_grad;
    if (s_rect) radam_chunk<RULE_RADAM_RECT>(k, o, tid);
    else radam_chunk<RULE_RADAM_PLAIN>(k, o, tid);
}

}  // namespace

extern "C" int fd_res_qsample_f32(const float *x_start, const float *x_input, const int64_t *t, const float *alphas_cumsum,
                                  const float *betas_cumsum, int T, const float *noise, const int64_t *seeds, int noise_step,
                                  int normalize, float *x_in, float *x_res, float *noise_out, float *times, int B, int64_t npix,
                                  void *stream) {
    FD_REQUIRE(x_start && x_input && t && alphas_cumsum && betas_cumsum && x_in && x_res && times, "fd_res_qsample_f32: null pointer");
    FD_REQUIRE((noise != nullptr) != (seeds != nullptr), "fd_res_qsample_f32: give either noise or seeds");
    FD_REQUIRE(!seeds || noise_out, "fd_res_qsample_f32: seeds need a noise_out");
    FD_REQUIRE(B > 0 && B <= 65535 && T > 0 && npix > 0 && npix < (1ll << 33),
               "fd_res_qsample_f32: unsupported shape B=%d T=%d npix=%lld (B <= 65535, npix < 2^33)", B, T, (long long)npix);
    const bool vec = npix % 4 == 0 && al16(x_start) && al16(x_input) && al16(noise) && al16(x_in) && al16(x_res) && al16(noise_out);
    const dim3 grid((unsigned)(((npix + 3) / 4 + 255) / 256), (unsigned)B);
#define FD_QS(V, K)                                                                                                            \
    hipLaunchKernelGGL((qsample_kernel<V, K>), grid, dim3(256), 0, (hipStream_t)stream, x_start, x_input, t, alphas_cumsum,      \
                       betas_cumsum, T, noise, seeds, noise_step, normalize, x_in, x_res, noise_out, times, B, npix)
    if (seeds) {
        if (vec) FD_QS(true, true);
        else FD_QS(false, true);
    } else {
        if (vec) FD_QS(true, false);
        else FD_QS(false, false);
    }
#undef FD_QS
    FD_LAUNCH_OK("fd_res_qsample_f32");
    return FD_OK;
}

extern "C" int64_t fd_res_loss_ws_floats(int B, int64_t npix) {
    if (B <= 0 || B > 65535 || npix <= 0 || npix >= (1ll << 40)) return 0;
    const int nchunk = ls_nchunk(npix), M1 = (nchunk + LS_G - 1) / LS_G;
    return round4((int64_t)B * nchunk) + round4((int64_t)B * M1);
}

extern "C" int fd_res_loss_f32(const float *pred, const float *target, int loss_type, double scale, float *loss, float *dpred,
                               float *ws, int B, int64_t npix, void *stream) {
    FD_REQUIRE(pred && target && loss && dpred && ws, "fd_res_loss_f32: null pointer");
    FD_REQUIRE(loss_type == 1 || loss_type == 2, "fd_res_loss_f32: loss_type must be 1 (l1) or 2 (l2) (got %d)", loss_type);
    FD_REQUIRE(fd_res_loss_ws_floats(B, npix) > 0, "fd_res_loss_f32: unsupported shape B=%d npix=%lld", B, (long long)npix);
    const hipStream_t st = (hipStream_t)stream;
    const int nchunk = ls_nchunk(npix), M1 = (nchunk + LS_G - 1) / LS_G;
    float *part = ws, *stage = part + round4((int64_t)B * nchunk);
    const bool vec = npix % 4 == 0 && al16(pred) && al16(target) && al16(dpred);
    const float c = (float)((loss_type == 2 ? 2.0 : 1.0) * scale / ((double)B * (double)npix));
    const dim3 grid((unsigned)nchunk, (unsigned)B);
#define FD_LS(V, Q) hipLaunchKernelGGL((loss_kernel<V, Q>), grid, dim3(256), 0, st, pred, target, dpred, part, npix, c)
    if (loss_type == 2) {
        if (vec) FD_LS(true, true);
        else FD_LS(false, true);
    } else {
        if (vec) FD_LS(true, false);
        else FD_LS(false, false);
    }
#undef FD_LS
    launch_sum(part, 1, nchunk, nchunk, 1, LS_G, stage, 1, M1, B, st);
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(256), 0, st, stage, M1, B, 1.0 / (double)npix, scale / (double)B, loss);
    FD_LAUNCH_OK("fd_res_loss_f32");
    return FD_OK;
}

extern "C" int fd_scale_dev_f32(const float *x, const float *s_dev, float *out, int64_t n, void *stream) {
    FD_REQUIRE(x && s_dev && out, "fd_scale_dev_f32: null pointer");
    FD_REQUIRE(n > 0 && n < (1ll << 40), "fd_scale_dev_f32: unsupported size n=%lld", (long long)n);
    const dim3 grid((unsigned)(((n + 3) / 4 + 255) / 256));
    if (al16(x) && al16(out)) hipLaunchKernelGGL(scale_dev_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, s_dev, out, n);
    else hipLaunchKernelGGL(scale_dev_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, s_dev, out, n);
    FD_LAUNCH_OK("fd_scale_dev_f32");
    return FD_OK;
}

extern "C" int fd_opt_chunk_elems(void) { return OPT_CHUNK; }

extern "C" int fd_opt_sumsq_f32(const int64_t *chunks, const int64_t *tensors, float *part, int nchunk, void *stream) {
    FD_REQUIRE(chunks && tensors && part, "fd_opt_sumsq_f32: null pointer");
    FD_REQUIRE(nchunk > 0, "fd_opt_sumsq_f32: no chunks (nchunk=%d)", nchunk);
    hipLaunchKernelGGL(opt_sumsq_kernel, dim3((unsigned)nchunk), dim3(256), 0, (hipStream_t)stream, chunks, tensors, part);
    FD_LAUNCH_OK("fd_opt_sumsq_f32");
    return FD_OK;
}

extern "C" int fd_opt_clip_coef(const float *part, int nchunk, const int64_t *tensors, int *steps, int nt, float max_norm,
                                int skip_nonfinite, float *rec, void *stream) {
    FD_REQUIRE(part && tensors && steps && rec, "fd_opt_clip_coef: null pointer");
    FD_REQUIRE(nchunk > 0 && nt > 0, "fd_opt_clip_coef: no chunks or tensors (nchunk=%d nt=%d)", nchunk, nt);
    hipLaunchKernelGGL(opt_clip_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, part, nchunk, tensors, steps, nt, max_norm,
                       skip_nonfinite, rec);
    FD_LAUNCH_OK("fd_opt_clip_coef");
    return FD_OK;
}

extern "C" int fd_opt_adam_ema_f32(const int64_t *chunks, const int64_t *tensors, const int *steps, const float *rec, int nchunk,
                                   double lr, double beta1, double beta2, double eps, int ema_mode, double ema_decay,
                                   int zero_grad, int skip_nonfinite, void *stream) {
    FD_REQUIRE(chunks && tensors && steps && rec, "fd_opt_adam_ema_f32: null pointer");
    FD_REQUIRE(nchunk > 0, "fd_opt_adam_ema_f32: no chunks (nchunk=%d)", nchunk);
    FD_REQUIRE(ema_mode >= 0 && ema_mode <= 2, "fd_opt_adam_ema_f32: ema_mode must be 0, 1 or 2 (got %d)", ema_mode);
    hipLaunchKernelGGL(opt_adam_kernel, dim3((unsigned)nchunk), dim3(256), 0, (hipStream_t)stream, chunks, tensors, steps, rec, lr,
                       beta1, beta2, eps, ema_mode, ema_decay, zero_grad, skip_nonfinite);
    FD_LAUNCH_OK("fd_opt_adam_ema_f32");
    return FD_OK;
}

extern "C" int fd_opt_radam_ema_f32(const int64_t *chunks, const int64_t *tensors, const int *steps, const float *rec, int nchunk,
                                    double lr, double beta1, double beta2, double eps, int ema_mode, double ema_decay,
                                    int zero_grad, int skip_nonfinite, void *stream) {
    FD_REQUIRE(chunks && tensors && steps && rec, "fd_opt_radam_ema_f32: null pointer");
    FD_REQUIRE(nchunk > 0, "fd_opt_radam_ema_f32: no chunks (nchunk=%d)", nchunk);
    FD_REQUIRE(ema_mode >= 0 && ema_mode <= 2, "fd_opt_radam_ema_f32: ema_mode must be 0, 1 or 2 (got %d)", ema_mode);
    hipLaunchKernelGGL(opt_radam_kernel, dim3((unsigned)nchunk), dim3(256), 0, (hipStream_t)stream, chunks, tensors, steps, rec, lr,
                       beta1, beta2, eps, ema_mode, ema_decay, zero_grad, skip_nonfinite);
    FD_LAUNCH_OK("fd_opt_radam_ema_f32");
    return FD_OK;
}
