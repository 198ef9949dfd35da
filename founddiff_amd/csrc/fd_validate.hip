// fd_validate.hip -- what a held-out evaluation reads off a model output (Trainer.validate; the reference has no counterpart: it
// runs its full test() every 10 000 steps, src/DADiff.py:1731-1745):
//
//   fd_val_items_f32       items[b] = (mean_i |pred - target| or (pred - target)^2, the one-step denoising error), one pass + two
//                          small sums, no gradient
//
// Column 0 is the per-slice mean whose batch mean is fd_res_loss_f32's loss (fd_train_step.hip; src/DADiff.py:1476-1481).  Column 1
// is the mean of (u(x0_hat) - u(x_start))^2 with x0_hat = clamp(x_input - clamp(pred, -1, 1), -1, 1), the samplers' last-step
// formula (src/DADiff.py:1203-1206, 1317-1318), and u(v) = clamp((v + 1) / 2, 0, 1), the [0, 1] units of compute_psnr /
// compute_rmse.  Since u(v) = (clamp(v, -1, 1) + 1) / 2, the difference is formed as (x0_hat - clamp(x_start, -1, 1)) / 2: the
// same number without the two roundings of v + 1.
//
// As the loss: no float atomics; grid (chunk, b), one partial pair per (b, chunk), added in index order (groups of LS_G in float,
// the groups in double), so a slice's row depends on npix and on nothing else in its batch.  Every lane owns the same elements on
// the 16-byte path and on the scalar path, and the arithmetic is written with explicit fmaf, so the two paths give the same bits.
#include "fd_train_common.h"

namespace {

constexpr int VL_CHUNK = 8192;         // pixels of a slice per workgroup: 256 lanes x 8 vectors of 4
constexpr int VL_VPL = VL_CHUNK / 1024;
constexpr int VL_G = 32;               // partials per launch_sum group

__device__ __forceinline__ float clamp1(float v) { return fminf(fmaxf(v, -1.f), 1.f); }

// grid (chunk of VL_CHUNK pixels, b): part[b][chunk] = (the chunk's sum of |d| or d^2, its sum of squared denoising errors)
template <bool VEC, bool L2, bool DENOISE>
__global__ __launch_bounds__(256) void val_items_kernel(const float *__restrict__ pred, const float *__restrict__ target,
                                                       const float *__restrict__ x_input, const float *__restrict__ x_start,
                                                       float *__restrict__ part, int64_t npix) {
    __shared__ float red0[256], red1[256];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int64_t base = (int64_t)b * npix, c0 = (int64_t)blockIdx.x * VL_CHUNK;
    float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
    for (int j = 0; j < VL_VPL; ++j) {
        const int64_t i0 = c0 + 4 * (j * 256 + tid);
        if (i0 >= npix) continue;
        const int n = (int)min((int64_t)4, npix - i0);
        float p[4], q[4], xi[4], x0[4];
        load4<VEC>(pred + base + i0, n, p);
        load4<VEC>(target + base + i0, n, q);
        if (DENOISE) {
            load4<VEC>(x_input + base + i0, n, xi);
            load4<VEC>(x_start + base + i0, n, x0);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float df = p[e] - q[e];                                // 0 - 0 past the end
            acc0 = L2 ? fmaf(df, df, acc0) : acc0 + fabsf(df);
            if (DENOISE) {
                const float hat = clamp1(xi[e] - clamp1(p[e]));          // 0 past the end, as clamp1(x0) is
                const float du = 0.5f * (hat - clamp1(x0[e]));
                acc1 = fmaf(du, du, acc1);
            }
        }
    }
    const float s0 = block_sum256(acc0, red0);
    const float s1 = DENOISE ? block_sum256(acc1, red1) : 0.f;
    if (tid == 0) {
        float *o = part + 2 * ((int64_t)b * gridDim.x + blockIdx.x);
        o[0] = s0;
        o[1] = s1;
    }
}

// grid (b / 256), one lane per slice: items[b] = the slice's M staged sums, added in index order in double, over npix; column 1
// is NaN when the call had no x_input / x_start
__global__ __launch_bounds__(256) void val_finish_kernel(const float *__restrict__ stage, int M, int B, double inv_npix, int denoise,
                                                        float *__restrict__ items) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const float *s = stage + 2 * (int64_t)b * M;
    double t0 = 0.0, t1 = 0.0;
    for (int m = 0; m < M; ++m) {
        t0 += (double)s[2 * m];
        t1 += (double)s[2 * m + 1];
    }
    items[2 * (int64_t)b] = (float)(t0 * inv_npix);
    items[2 * (int64_t)b + 1] = denoise ? (float)(t1 * inv_npix) : __builtin_nanf("");
}

int vl_nchunk(int64_t npix) { return (int)((npix + VL_CHUNK - 1) / VL_CHUNK); }

}  // namespace

extern "C" int64_t fd_val_items_ws_floats(int B, int64_t npix) {
    if (B <= 0 || B > 65535 || npix <= 0 || npix >= (1ll << 40)) return 0;
    const int nchunk = vl_nchunk(npix), M1 = (nchunk + VL_G - 1) / VL_G;
    return round4(2 * (int64_t)B * nchunk) + round4(2 * (int64_t)B * M1);
}

extern "C" int fd_val_items_f32(const float *pred, const float *target, const float *x_input, const float *x_start, int loss_type,
                                float *items, float *ws, int B, int64_t npix, void *stream) {
    FD_REQUIRE(pred && target && items && ws, "fd_val_items_f32: null pointer");
    FD_REQUIRE((x_input != nullptr) == (x_start != nullptr), "fd_val_items_f32: give both x_input and x_start, or neither");
    FD_REQUIRE(loss_type == 1 || loss_type == 2, "fd_val_items_f32: loss_type must be 1 (l1) or 2 (l2) (got %d)", loss_type);
    FD_REQUIRE(fd_val_items_ws_floats(B, npix) > 0, "fd_val_items_f32: unsupported shape B=%d npix=%lld", B, (long long)npix);
    const hipStream_t st = (hipStream_t)stream;
    const int nchunk = vl_nchunk(npix), M1 = (nchunk + VL_G - 1) / VL_G;
    float *part = ws, *stage = part + round4(2 * (int64_t)B * nchunk);
    const bool denoise = x_input != nullptr;
    const bool vec = npix % 4 == 0 && al16(pred) && al16(target) && al16(x_input) && al16(x_start);
    const dim3 grid((unsigned)nchunk, (unsigned)B);
#define FD_VL(V, Q, D) \
    hipLaunchKernelGGL((val_items_kernel<V, Q, D>), grid, dim3(256), 0, st, pred, target, x_input, x_start, part, npix)
#define FD_VL_D(V, Q)         \
    do {                      \
        if (denoise) FD_VL(V, Q, true); \
        else FD_VL(V, Q, false);        \
    } while (0)
    if (loss_type == 2) {
        if (vec) FD_VL_D(true, true);
        else FD_VL_D(false, true);
    } else {
        if (vec) FD_VL_D(true, false);
        else FD_VL_D(false, false);
    }
#undef FD_VL_D
#undef FD_VL
    // part [B][nchunk][2] -> stage [B][M1][2]: groups of VL_G chunks, both columns
    launch_sum(part, 2, 2 * (int64_t)nchunk, nchunk, 2, VL_G, stage, 2, 2 * (int64_t)M1, B, st);
    hipLaunchKernelGGL(val_finish_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, stage, M1, B, 1.0 / (double)npix,
                       (int)denoise, items);
    FD_LAUNCH_OK("fd_val_items_f32");
    return FD_OK;
}
