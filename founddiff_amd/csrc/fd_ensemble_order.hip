// fd_ensemble_order.hip -- per-pixel order statistics of an ensemble's K final images and the coverage of a target by two of the maps
// (ResidualDiffusion.sample_ensemble(quantiles=...); metrics.ensemble_quantiles, metrics.interval_coverage).  fp32, the same code in
// both builds of the library; no float atomics.
//
//   fd_ensemble_order_f32     samples [B][K][n] -> out [B][Q][n]: per pixel, with its K values in ascending order v_(0) <= ... <=
//                             v_(K-1), level j is fmaf(frac[j], v_(hi[j]) - v_(lo[j]), v_(lo[j])), and v_(lo[j]) itself where
//                             frac[j] == 0.  The table comes by value in the kernel's arguments: no device table, no upload.
//   fd_ensemble_coverage_f32  count[b] = the number of pixels with lo_map <= target <= hi_map, exactly.
//
// An order statistic is a selection, so HOW the K values are ordered cannot show in the result: two paths, the same bits.
//   K <= 32: a sorting network in registers (Batcher's merge exchange, Knuth 5.2.2 M) instantiated for 4 / 8 / 16 / 32 values, the
//            tail padded with +inf.  Every index is a compile-time constant, every sample is read once, and rank r is picked out
//            of the sorted registers by comparing r with each constant index (the table is wave-uniform).
//   K > 32:  selection by counting.  rank(v_i) = #{j : v_j < v_i or (v_j == v_i and j < i)} is a permutation of 0 .. K-1; the value
//            whose rank is lo[j] (hi[j]) is v_(lo[j]) (v_(hi[j])).  Four candidates at a time against all K values, which are
//            re-read from the L2 the workgroup has just filled, as the second pass of ensemble_stats_kernel does: K^2 / 4 vector loads
//            per lane and no array indexed by k.
// Equal values are interchangeable (-0 and +0 compare equal: either may come back).  v_min_f32 / v_max_f32 and the counting
// comparisons both lose a NaN, so a pixel's NaNs are found as the values are read and every level of that pixel is NaN.
// A lane owns the 4 consecutive flat pixels that it owns in ensemble_stats_kernel, on the 16-byte path and on the scalar path, and
// a pixel's result is a function of its own K values and the table: nothing depends on B, the other slices or the grid.
#include <math.h>
#include "fd_train_common.h"

namespace {

constexpr int EO_CHUNK = 1024;         // pixels of a slice per workgroup: 256 lanes x one vector of 4 (fd_ensemble.hip's ES_CHUNK)
constexpr int EO_QMAX = 8;             // levels per call
constexpr int EO_NET_MAX = 32;         // the largest K the networks serve
constexpr int EO_KMAX = 65535;
constexpr int EO_CB = 4;               // candidates per sweep of the counting path

struct OrderTable {
    int lo[EO_QMAX], hi[EO_QMAX];
    float frac[EO_QMAX];
};

__device__ __forceinline__ float eo_level(float a, float b, float frac, bool nan) {
    const float v = frac == 0.f ? a : fmaf(frac, b - a, a);
    return nan ? __builtin_nanf("") : v;
}

// grid (chunk of EO_CHUNK pixels, b); P: the padded size, K <= P
template <bool VEC, int P>
__global__ __launch_bounds__(256) void order_net_kernel(const float *__restrict__ x, float *__restrict__ out, OrderTable tab, int K,
                                                       int Q, int64_t n) {
    const int b = blockIdx.y;
    const int64_t i0 = (int64_t)blockIdx.x * EO_CHUNK + 4 * threadIdx.x;
    if (i0 >= n) return;
    const int m = (int)min((int64_t)4, n - i0);
    const float *xp = x + (int64_t)b * K * n + i0;
    float v[P][4];
    bool nan[4] = {false, false, false, false};
#pragma unroll
    for (int k = 0; k < P; ++k) {
        if (k < K) {
            load4<VEC>(xp + (int64_t)k * n, m, v[k]);
#pragma unroll
            for (int e = 0; e < 4; ++e) nan[e] |= v[k][e] != v[k][e];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[k][e] = INFINITY;
        }
    }
    // merge exchange: p the run length being merged, k the comparator distance
#pragma unroll
    for (int p = 1; p < P; p *= 2)
#pragma unroll
        for (int k = p; k >= 1; k /= 2)
#pragma unroll
            for (int j = k % p; j + k < P; j += 2 * k)
#pragma unroll
                for (int i = 0; i < k; ++i) {
                    const int s = i + j, t = i + j + k;
                    if (t < P && s / (2 * p) == t / (2 * p)) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float a = v[s][e], c = v[t][e];
                            v[s][e] = fminf(a, c);
                            v[t][e] = fmaxf(a, c);
                        }
                    }
                }
    float *op = out + (int64_t)b * Q * n + i0;
    for (int q = 0; q < Q; ++q) {
        const int rl = tab.lo[q], rh = tab.hi[q];
        float a[4], c[4], o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] = c[e] = v[0][e];
#pragma unroll
        for (int k = 1; k < P; ++k) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a[e] = rl == k ? v[k][e] : a[e];
                c[e] = rh == k ? v[k][e] : c[e];
            }
        }
        const float f = tab.frac[q];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = eo_level(a[e], c[e], f, nan[e]);
        store4<VEC>(op + (int64_t)q * n, m, o);
    }
}

// grid (chunk of EO_CHUNK pixels, b); any K
template <bool VEC>
__global__ __launch_bounds__(256) void order_rank_kernel(const float *__restrict__ x, float *__restrict__ out, OrderTable tab, int K,
                                                        int Q, int64_t n) {
    const int b = blockIdx.y;
    const int64_t i0 = (int64_t)blockIdx.x * EO_CHUNK + 4 * threadIdx.x;
    if (i0 >= n) return;
    const int m = (int)min((int64_t)4, n - i0);
    const float *xp = x + (int64_t)b * K * n + i0;
    float a[EO_QMAX][4], c[EO_QMAX][4];
#pragma unroll
    for (int q = 0; q < EO_QMAX; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) a[q][e] = c[q][e] = 0.f;
    bool nan[4] = {false, false, false, false};
    for (int c0 = 0; c0 < K; c0 += EO_CB) {
        // candidates c0 .. c0 + 3; one past the end repeats the last value under a rank that no level asks for
        float vi[EO_CB][4];
        int rank[EO_CB][4];
#pragma unroll
        for (int t = 0; t < EO_CB; ++t) {
            load4<VEC>(xp + (int64_t)min(c0 + t, K - 1) * n, m, vi[t]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                nan[e] |= vi[t][e] != vi[t][e];
                rank[t][e] = 0;
            }
        }
        for (int j = 0; j < K; ++j) {
            float vj[4];
            load4<VEC>(xp + (int64_t)j * n, m, vj);
#pragma unroll
            for (int t = 0; t < EO_CB; ++t) {
                const bool before = j < c0 + t;                          // wave-uniform: ties go to the smaller index
#pragma unroll
                for (int e = 0; e < 4; ++e) rank[t][e] += (before ? vj[e] <= vi[t][e] : vj[e] < vi[t][e]) ? 1 : 0;
            }
        }
#pragma unroll
        for (int t = 0; t < EO_CB; ++t) {
            const bool live = c0 + t < K;
#pragma unroll
            for (int q = 0; q < EO_QMAX; ++q) {
                if (q < Q) {
                    const int rl = live ? tab.lo[q] : -1, rh = live ? tab.hi[q] : -1;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        a[q][e] = rank[t][e] == rl ? vi[t][e] : a[q][e];
                        c[q][e] = rank[t][e] == rh ? vi[t][e] : c[q][e];
                    }
                }
            }
        }
    }
    float *op = out + (int64_t)b * Q * n + i0;
#pragma unroll
    for (int q = 0; q < EO_QMAX; ++q) {
        if (q < Q) {
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = eo_level(a[q][e], c[q][e], tab.frac[q], nan[e]);
            store4<VEC>(op + (int64_t)q * n, m, o);
        }
    }
}

// the sum of v over the 256 lanes; red: 256 ints of LDS
__device__ __forceinline__ int block_count256(int v, int *red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// grid (chunk of EO_CHUNK pixels, b): part[b][chunk] = the chunk's pixels with lo <= target <= hi (a NaN compares false)
template <bool VEC>
__global__ __launch_bounds__(256) void coverage_kernel(const float *__restrict__ lo, int64_t lo_bs, const float *__restrict__ hi,
                                                      int64_t hi_bs, const float *__restrict__ tg, int64_t tg_bs,
                                                      int *__restrict__ part, int nchunk, int64_t n) {
    __shared__ int red[256];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int64_t i0 = (int64_t)blockIdx.x * EO_CHUNK + 4 * tid;
    int cnt = 0;
    if (i0 < n) {
        const int m = (int)min((int64_t)4, n - i0);
        float l[4], h[4], t[4];
        load4<VEC>(lo + (int64_t)b * lo_bs + i0, m, l);
        load4<VEC>(hi + (int64_t)b * hi_bs + i0, m, h);
        load4<VEC>(tg + (int64_t)b * tg_bs + i0, m, t);
#pragma unroll
        for (int e = 0; e < 4; ++e) cnt += (e < m && l[e] <= t[e] && t[e] <= h[e]) ? 1 : 0;
    }
    const int s = block_count256(cnt, red);
    if (tid == 0) part[(int64_t)b * nchunk + blockIdx.x] = s;
}

// grid (b / 256), one lane per slice: count[b] = the slice's chunk counts, added in index order
__global__ __launch_bounds__(256) void coverage_finish_kernel(const int *__restrict__ part, int nchunk, int B,
                                                             int64_t *__restrict__ count) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const int *p = part + (int64_t)b * nchunk;
    int64_t t = 0;
    for (int m = 0; m < nchunk; ++m) t += p[m];
    count[b] = t;
}

int eo_nchunk(int64_t n) { return (int)((n + EO_CHUNK - 1) / EO_CHUNK); }

bool eo_shape_ok(int64_t n) { return n > 0 && n < (1ll << 40); }

template <bool VEC>
void order_launch(const float *x, float *out, const OrderTable &tab, int B, int K, int Q, int64_t n, hipStream_t st) {
    const dim3 grid((unsigned)eo_nchunk(n), (unsigned)B);
    if (K <= 4) hipLaunchKernelGGL((order_net_kernel<VEC, 4>), grid, dim3(256), 0, st, x, out, tab, K, Q, n);
    else if (K <= 8) hipLaunchKernelGGL((order_net_kernel<VEC, 8>), grid, dim3(256), 0, st, x, out, tab, K, Q, n);
    else if (K <= 16) hipLaunchKernelGGL((order_net_kernel<VEC, 16>), grid, dim3(256), 0, st, x, out, tab, K, Q, n);
    else if (K <= EO_NET_MAX) hipLaunchKernelGGL((order_net_kernel<VEC, 32>), grid, dim3(256), 0, st, x, out, tab, K, Q, n);
    else hipLaunchKernelGGL(order_rank_kernel<VEC>, grid, dim3(256), 0, st, x, out, tab, K, Q, n);
}

}  // namespace

extern "C" int fd_ensemble_order_f32(const float *samples, float *out, const int *lo, const int *hi, const float *frac, int B, int K,
                                     int Q, int64_t n, void *stream) {
    FD_REQUIRE(samples && out && lo && hi && frac, "fd_ensemble_order_f32: null pointer");
    FD_REQUIRE(B > 0 && B <= 65535 && K > 0 && K <= EO_KMAX && Q > 0 && Q <= EO_QMAX && eo_shape_ok(n),
               "fd_ensemble_order_f32: unsupported shape B=%d K=%d Q=%d n=%lld", B, K, Q, (long long)n);
    OrderTable tab = {};
    for (int q = 0; q < Q; ++q) {
        FD_REQUIRE(0 <= lo[q] && lo[q] <= hi[q] && hi[q] <= K - 1 && frac[q] >= 0.f && frac[q] <= 1.f,
                   "fd_ensemble_order_f32: bad table row %d: lo=%d hi=%d frac=%g (0 <= lo <= hi <= K-1 = %d, 0 <= frac <= 1)", q, lo[q],
                   hi[q], (double)frac[q], K - 1);
        tab.lo[q] = lo[q];
        tab.hi[q] = hi[q];
        tab.frac[q] = frac[q];
    }
    if (n % 4 == 0 && al16(samples) && al16(out)) order_launch<true>(samples, out, tab, B, K, Q, n, (hipStream_t)stream);
    else order_launch<false>(samples, out, tab, B, K, Q, n, (hipStream_t)stream);
    FD_LAUNCH_OK("fd_ensemble_order_f32");
    return FD_OK;
}

// ints of workspace per slice: its chunk counts
extern "C" int fd_ensemble_coverage_nblk(int64_t n) { return eo_shape_ok(n) ? eo_nchunk(n) : 0; }

extern "C" int fd_ensemble_coverage_f32(const float *lo_map, int64_t lo_bstride, const float *hi_map, int64_t hi_bstride,
                                        const float *target, int64_t target_bstride, int *ws, int64_t *count, int B, int64_t n,
                                        void *stream) {
    FD_REQUIRE(lo_map && hi_map && target && ws && count, "fd_ensemble_coverage_f32: null pointer");
    FD_REQUIRE(B > 0 && B <= 65535 && eo_shape_ok(n) && lo_bstride >= 0 && hi_bstride >= 0 && target_bstride >= 0,
               "fd_ensemble_coverage_f32: unsupported shape B=%d n=%lld strides %lld %lld %lld", B, (long long)n,
               (long long)lo_bstride, (long long)hi_bstride, (long long)target_bstride);
    const hipStream_t st = (hipStream_t)stream;
    const int nchunk = eo_nchunk(n);
    const bool vec = n % 4 == 0 && al16(lo_map) && al16(hi_map) && al16(target) && lo_bstride % 4 == 0 && hi_bstride % 4 == 0 &&
                     target_bstride % 4 == 0;
    const dim3 grid((unsigned)nchunk, (unsigned)B);
    if (vec)
        hipLaunchKernelGGL(coverage_kernel<true>, grid, dim3(256), 0, st, lo_map, lo_bstride, hi_map, hi_bstride, target,
                           target_bstride, ws, nchunk, n);
    else
        hipLaunchKernelGGL(coverage_kernel<false>, grid, dim3(256), 0, st, lo_map, lo_bstride, hi_map, hi_bstride, target,
                           target_bstride, ws, nchunk, n);
    hipLaunchKernelGGL(coverage_finish_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, ws, nchunk, B, count);
    FD_LAUNCH_OK("fd_ensemble_coverage_f32");
    return FD_OK;
}
