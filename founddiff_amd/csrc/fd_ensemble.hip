// fd_ensemble.hip -- what an ensemble of K keyed realisations per slice needs around the samplers (ResidualDiffusion.sample_ensemble;
// the reference has no counterpart: it denoises every slice once).  fp32, the same code in both builds of the library.
//
//   fd_rows_repeat_f32     dst[b K + k] = src[b]: a slice's input plane and its conditioning rows, once per replica.  One read and K
//                          writes per element.
//   fd_ensemble_stats_f32  per pixel the mean and the sample standard deviation over a slice's K final images, per slice the
//                          spread = sqrt(mean over pixels of std^2).
//
// The statistics are two passes over k, both in k order: mean = (x_0 + x_1 + ... ) / K, then v = sum (x_k - mean)^2 / (K - 1) with
// fmaf, std = sqrt(v); K = 1 gives std = 0 exactly.  (E[x^2] - mean^2 in fp32 is 40 % wrong at mean 0.5, sigma 1e-3.)  The second
// pass re-reads the K values: a workgroup's K x 4 KB are in the L2 it has just filled, so HBM sees K reads and two writes per pixel.
// The spread is summed as the loss is: no float atomics; grid (chunk, b), one partial per (b, chunk) from block_sum256, the partials
// of a slice added in index order (groups of ES_G in float, the groups in double), so a slice's rows depend on K and n and on
// nothing else in the launch.  Every lane owns the same elements on the 16-byte path and on the scalar path and the arithmetic is
// written with explicit fmaf, so the two paths give the same bits.
#include "fd_train_common.h"

namespace {

constexpr int ES_CHUNK = 1024;         // pixels of a slice per workgroup: 256 lanes x one vector of 4
constexpr int ES_G = 32;               // partials per launch_sum group

// grid (block of 256 vectors, b in steps of gridDim.y)
template <bool VEC>
__global__ __launch_bounds__(256) void rows_repeat_kernel(const float *__restrict__ src, float *__restrict__ dst, int B, int K,
                                                         int64_t n) {
    const int64_t i0 = 4 * ((int64_t)blockIdx.x * 256 + threadIdx.x);
    if (i0 >= n) return;
    const int m = (int)min((int64_t)4, n - i0);
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        float v[4];
        load4<VEC>(src + (int64_t)b * n + i0, m, v);
        float *d = dst + (int64_t)b * K * n + i0;
        for (int k = 0; k < K; ++k) store4<VEC>(d + (int64_t)k * n, m, v);
    }
}

// grid (chunk of ES_CHUNK pixels, b): mean, std of the chunk's pixels; part[b][chunk] = the chunk's sum of std^2
template <bool VEC>
__global__ __launch_bounds__(256) void ensemble_stats_kernel(const float *__restrict__ x, float *__restrict__ mean,
                                                            float *__restrict__ sd, float *__restrict__ part, int64_t part_bstride,
                                                            int K, int64_t n) {
    __shared__ float red[256];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int64_t i0 = (int64_t)blockIdx.x * ES_CHUNK + 4 * tid;
    float acc = 0.f;
    if (i0 < n) {
        const int m = (int)min((int64_t)4, n - i0);
        const float *xp = x + (int64_t)b * K * n + i0;
        float s[4] = {0.f, 0.f, 0.f, 0.f}, v[4], mu[4], q[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
        for (int k = 0; k < K; ++k) {
            load4<VEC>(xp + (int64_t)k * n, m, v);
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] += v[e];
        }
        const float fk = (float)K;
#pragma unroll
        for (int e = 0; e < 4; ++e) mu[e] = s[e] / fk;
        for (int k = 0; k < K; ++k) {
            load4<VEC>(xp + (int64_t)k * n, m, v);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = v[e] - mu[e];
                q[e] = fmaf(d, d, q[e]);
            }
        }
        const float fk1 = (float)(K - 1);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float var = K > 1 ? q[e] / fk1 : 0.f;                  // 0 past the end: 0 - 0
            o[e] = sqrtf(var);
            acc += var;
        }
        store4<VEC>(mean + (int64_t)b * n + i0, m, mu);
        store4<VEC>(sd + (int64_t)b * n + i0, m, o);
    }
    const float t = block_sum256(acc, red);
    if (tid == 0) part[(int64_t)b * part_bstride + blockIdx.x] = t;
}

// grid (b / 256), one lane per slice: spread[b] = sqrt(the slice's M staged sums, added in index order in double, over n)
__global__ __launch_bounds__(256) void ensemble_finish_kernel(const float *__restrict__ stage, int64_t stage_bstride, int M, int B,
                                                             double inv_n, float *__restrict__ spread) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const float *s = stage + (int64_t)b * stage_bstride;
    double t = 0.0;
    for (int m = 0; m < M; ++m) t += (double)s[m];
    spread[b] = (float)sqrt(t * inv_n);
}

int es_nchunk(int64_t n) { return (int)((n + ES_CHUNK - 1) / ES_CHUNK); }

bool es_shape_ok(int64_t n) { return n > 0 && n < (1ll << 40); }

}  // namespace

// floats of workspace per slice: its chunk partials, then its staged group sums
extern "C" int fd_ensemble_nblk(int64_t n) {
    if (!es_shape_ok(n)) return 0;
    const int nchunk = es_nchunk(n);
    return nchunk + (nchunk + ES_G - 1) / ES_G;
}

extern "C" int fd_rows_repeat_f32(const float *src, float *dst, int B, int K, int64_t n, void *stream) {
    FD_REQUIRE(src && dst, "fd_rows_repeat_f32: null pointer");
    FD_REQUIRE(B > 0 && K > 0 && es_shape_ok(n), "fd_rows_repeat_f32: unsupported shape B=%d K=%d n=%lld", B, K, (long long)n);
    const bool vec = n % 4 == 0 && al16(src) && al16(dst);
    const dim3 grid((unsigned)cdiv((n + 3) / 4, 256), (unsigned)min(B, 65535));
    if (vec) hipLaunchKernelGGL(rows_repeat_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, src, dst, B, K, n);
    else hipLaunchKernelGGL(rows_repeat_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, src, dst, B, K, n);
    FD_LAUNCH_OK("fd_rows_repeat_f32");
    return FD_OK;
}

extern "C" int fd_ensemble_stats_f32(const float *samples, float *mean, float *std, float *ws, float *spread, int B, int K,
                                     int64_t n, void *stream) {
    FD_REQUIRE(samples && mean && std && ws && spread, "fd_ensemble_stats_f32: null pointer");
    FD_REQUIRE(B > 0 && B <= 65535 && K > 0 && es_shape_ok(n), "fd_ensemble_stats_f32: unsupported shape B=%d K=%d n=%lld", B, K,
               (long long)n);
    const hipStream_t st = (hipStream_t)stream;
    const int nchunk = es_nchunk(n), M1 = (nchunk + ES_G - 1) / ES_G;
    const int64_t nblk = nchunk + M1;
    float *part = ws, *stage = ws + nchunk;                              // per slice: [nchunk partials][M1 staged sums]
    const bool vec = n % 4 == 0 && al16(samples) && al16(mean) && al16(std);
    const dim3 grid((unsigned)nchunk, (unsigned)B);
    if (vec) hipLaunchKernelGGL(ensemble_stats_kernel<true>, grid, dim3(256), 0, st, samples, mean, std, part, nblk, K, n);
    else hipLaunchKernelGGL(ensemble_stats_kernel<false>, grid, dim3(256), 0, st, samples, mean, std, part, nblk, K, n);
    launch_sum(part, 1, nblk, nchunk, 1, ES_G, stage, 1, nblk, B, st);
    hipLaunchKernelGGL(ensemble_finish_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, stage, nblk, M1, B,
                       1.0 / (double)n, spread);
    FD_LAUNCH_OK("fd_ensemble_stats_f32");
    return FD_OK;
}
