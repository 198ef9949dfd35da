// fd_interval.hip -- calibrated ensemble intervals (metrics.interval_hist, metrics.interval_scale; Trainer.calibrate_intervals and
// Trainer.test(interval_scale=...); the reference has no counterpart).  fp32, the same code in both builds of the library; no float
// atomics, no atomics on global memory.
//
//   fd_interval_hist_f32   per slice the histogram over a grid of scales of the pixel score
//                              d_lo = fmaxf(m - l, floor)   d_hi = fmaxf(u - m, floor)   s = fmaxf((m - y) / d_lo, (y - m) / d_hi),
//                          the smallest scale whose interval [m - s d_lo, m + s d_hi] holds the target y.  Every difference and every
//                          quotient is one correctly rounded fp32 operation (contraction is off; the division is the IEEE one), so
//                          numpy float32 gives the same bits.  bin = the number of grid values strictly below s (s == grid[g] -> g);
//                          a pixel with a NaN among m, l, u, y or in either quotient is covered at no scale and goes to bin G, where
//                          s = +inf arrives by itself.
//   fd_interval_scale_f32  lo_out = clamp(m - scale d_lo, 0, 1), hi_out = clamp(m + scale d_hi, 0, 1), the product and the sum two
//                          roundings, and per slice width = mean over pixels of hi_out - lo_out.
//
// The histogram: grid (p, b), P = min(chunks, IV_P) workgroups per slice, workgroup p walks chunks p, p + P, ... of 1024 pixels.  The
// scale grid (G floats) and the workgroup's counters (bins 0 .. G - 1) sit in LDS, 2 x 16 KB; bin G is a per-wave register count
// (ballot + popcount), parked in the grid's LDS once the walk is over.  A pixel's bin is a branch-free binary search, ceil(log2(G + 1))
// LDS reads with the same trip count in every lane.  Counters are integers: any order of addition is exact.
// Contention: a CT slice is a third air, where every map is 0, s = 0 and the bin is 0, so one LDS counter would take a third of
// all ds_add, which the LDS serialises per address.  Per vector element a wave therefore settles its two most common-looking bins by
// ballot: the first live lane's bin, then the first remaining lane's -- one ds_add of the popcount each -- and only lanes left after
// that add 1 on their own.  A wave in air issues 4 adds for its 256 pixels, a wave on the air / tissue edge settles both sides.
// Each workgroup writes its G + 1 counts to part[b][p][.]; the finish kernel adds a slice's P rows in index order into int64.
// A slice's P depends on n alone, a lane owns the same 4 pixels on the 16-byte and on the scalar path: same counts either way, in
// any batch.
//
// The width is summed as fd_ensemble_stats_f32 sums its spread: one fp32 partial per (b, chunk) from block_sum256, a slice's partials
// added in index order in double.  A NaN in m, l or u makes both outputs NaN at that pixel and nowhere else, and the slice's width NaN.
#include <math.h>
#include "fd_train_common.h"

namespace {

constexpr int IV_CHUNK = 1024;         // pixels of a slice per workgroup pass: 256 lanes x one vector of 4
constexpr int IV_GMAX = 4096;          // grid values per call: 16 KB of LDS, and 16 KB of counters
constexpr int IV_P = 64;               // histogram workgroups per slice at most

__device__ __forceinline__ bool iv_nan(float v) { return v != v; }

// the half-widths of a pixel
__device__ __forceinline__ void iv_half_widths(float m, float l, float u, float floor, float &d_lo, float &d_hi) {
#pragma clang fp contract(off)
    d_lo = fmaxf(m - l, floor);
    d_hi = fmaxf(u - m, floor);
}

// the score of a pixel; `out` where no scale covers it for want of a number
__device__ __forceinline__ float iv_score(float m, float l, float u, float y, float floor, bool &out) {
#pragma clang fp contract(off)
    float d_lo, d_hi;
    iv_half_widths(m, l, u, floor, d_lo, d_hi);
    const float a = (m - y) / d_lo, b = (y - m) / d_hi;
    out = iv_nan(m) || iv_nan(l) || iv_nan(u) || iv_nan(y) || iv_nan(a) || iv_nan(b);
    return fmaxf(a, b);
}

// one count for every live lane's bin in h (LDS), called by the whole wave; the lanes that share the first live lane's bin, then
// those that share the first remaining lane's, are added once each
__device__ __forceinline__ void iv_wave_add(unsigned *h, int bin, bool live, int lane) {
    unsigned long long todo = __ballot(live);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (todo == 0) break;                                            // wave-uniform
        const int lead = __ffsll((long long)todo) - 1;
        const int lb = __builtin_amdgcn_readlane(bin, lead);
        const unsigned long long same = __ballot(live && bin == lb) & todo;
        if (lane == lead) atomicAdd(&h[lb], (unsigned)__popcll(same));
        todo &= ~same;
    }
    if ((todo >> lane) & 1) atomicAdd(&h[bin], 1u);
}

// grid (p, b): part[b][p][0 .. G] = the counts of chunks p, p + P, ... of slice b
template <bool VEC>
__global__ __launch_bounds__(256) void interval_hist_kernel(const float *__restrict__ ce, int64_t ce_bs, const float *__restrict__ lo,
                                                           int64_t lo_bs, const float *__restrict__ hi, int64_t hi_bs,
                                                           const float *__restrict__ tg, int64_t tg_bs,
                                                           const float *__restrict__ grid, int G, int P2, float floor,
                                                           int *__restrict__ part, int nchunk, int64_t n) {
    __shared__ float sg[IV_GMAX];
    __shared__ unsigned sh[IV_GMAX];
    const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.y, P = gridDim.x;
    for (int j = tid; j < G; j += 256) {
        sg[j] = grid[j];
        sh[j] = 0u;
    }
    __syncthreads();
    unsigned over = 0;                                                   // this wave's pixels of bin G: the same in its 64 lanes
    for (int c = blockIdx.x; c < nchunk; c += P) {
        const int64_t i0 = (int64_t)c * IV_CHUNK + 4 * tid;
        const int m = i0 < n ? (int)min((int64_t)4, n - i0) : 0;
        float vm[4], vl[4], vu[4], vy[4];
        if (m > 0) {
            load4<VEC>(ce + (int64_t)b * ce_bs + i0, m, vm);
            load4<VEC>(lo + (int64_t)b * lo_bs + i0, m, vl);
            load4<VEC>(hi + (int64_t)b * hi_bs + i0, m, vu);
            load4<VEC>(tg + (int64_t)b * tg_bs + i0, m, vy);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) vm[e] = vl[e] = vu[e] = vy[e] = 0.f;
        }
        int bin[4];
        bool out[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float s = iv_score(vm[e], vl[e], vu[e], vy[e], floor, out[e]);
            int pos = 0;                                                 // the number of grid values below s
            for (int step = P2; step > 0; step >>= 1) {
                const int t = pos + step;
                if (t <= G && sg[t - 1] < s) pos = t;
            }
            bin[e] = pos;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool live = e < m;
            const bool top = live && (out[e] || bin[e] == G);
            over += (unsigned)__popcll(__ballot(top));
            iv_wave_add(sh, bin[e], live && !top, lane);
        }
    }
    __syncthreads();                                                     // the grid is read no more: its first 4 words take the waves' bin G
    unsigned *so = (unsigned *)sg;
    if (lane == 0) so[tid >> 6] = over;
    __syncthreads();
    int *pp = part + ((int64_t)b * P + blockIdx.x) * (G + 1);
    for (int j = tid; j < G; j += 256) pp[j] = (int)sh[j];
    if (tid == 0) pp[G] = (int)(so[0] + so[1] + so[2] + so[3]);
}

// grid (bins / 256, b): hist[b][j] = the slice's P rows of part, added in index order
__global__ __launch_bounds__(256) void interval_hist_finish_kernel(const int *__restrict__ part, int P, int G1,
                                                                  int64_t *__restrict__ hist) {
    const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (j >= G1) return;
    const int *p = part + (int64_t)b * P * G1 + j;
    int64_t t = 0;
    for (int q = 0; q < P; ++q) t += p[(int64_t)q * G1];
    hist[(int64_t)b * G1 + j] = t;
}

// grid (chunk of IV_CHUNK pixels, b): the scaled maps of the chunk; part[b][chunk] = its sum of hi_out - lo_out
template <bool VEC>
__global__ __launch_bounds__(256) void interval_scale_kernel(const float *__restrict__ ce, int64_t ce_bs, const float *__restrict__ lo,
                                                            int64_t lo_bs, const float *__restrict__ hi, int64_t hi_bs, float scale,
                                                            float floor, float *__restrict__ lo_out, float *__restrict__ hi_out,
                                                            float *__restrict__ part, int nchunk, int64_t n) {
#pragma clang fp contract(off)
    __shared__ float red[256];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int64_t i0 = (int64_t)blockIdx.x * IV_CHUNK + 4 * tid;
    float acc = 0.f;
    if (i0 < n) {
        const int m = (int)min((int64_t)4, n - i0);
        float vm[4], vl[4], vu[4], ol[4], oh[4];
        load4<VEC>(ce + (int64_t)b * ce_bs + i0, m, vm);
        load4<VEC>(lo + (int64_t)b * lo_bs + i0, m, vl);
        load4<VEC>(hi + (int64_t)b * hi_bs + i0, m, vu);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float d_lo, d_hi;
            iv_half_widths(vm[e], vl[e], vu[e], floor, d_lo, d_hi);
            const float pl = scale * d_lo, ph = scale * d_hi;
            const float a = vm[e] - pl, c = vm[e] + ph;
            const bool nan = iv_nan(vm[e]) || iv_nan(vl[e]) || iv_nan(vu[e]);
            ol[e] = nan ? __builtin_nanf("") : fminf(fmaxf(a, 0.f), 1.f);
            oh[e] = nan ? __builtin_nanf("") : fminf(fmaxf(c, 0.f), 1.f);
            const float w = oh[e] - ol[e];
            acc += e < m ? w : 0.f;
        }
        store4<VEC>(lo_out + (int64_t)b * n + i0, m, ol);
        store4<VEC>(hi_out + (int64_t)b * n + i0, m, oh);
    }
    const float t = block_sum256(acc, red);
    if (tid == 0) part[(int64_t)b * nchunk + blockIdx.x] = t;
}

// grid (b / 256), one lane per slice: width[b] = the slice's chunk sums, added in index order in double, over n
__global__ __launch_bounds__(256) void interval_width_kernel(const float *__restrict__ part, int nchunk, int B, double inv_n,
                                                            float *__restrict__ width) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const float *p = part + (int64_t)b * nchunk;
    double t = 0.0;
    for (int m = 0; m < nchunk; ++m) t += (double)p[m];
    width[b] = (float)(t * inv_n);
}

int64_t iv_nchunk(int64_t n) { return (n + IV_CHUNK - 1) / IV_CHUNK; }

// a workgroup of the histogram counts at most n / IV_P + IV_CHUNK pixels in an int
bool iv_shape_ok(int64_t n) { return n > 0 && n < (1ll << 34); }

bool iv_strides_ok(int64_t a, int64_t b, int64_t c) { return a >= 0 && b >= 0 && c >= 0; }

}  // namespace

// histogram workgroups per slice; ws of fd_interval_hist_f32: B * this * (G + 1) ints
extern "C" int fd_interval_hist_nblk(int64_t n) { return iv_shape_ok(n) ? (int)min((int64_t)IV_P, iv_nchunk(n)) : 0; }

extern "C" int fd_interval_hist_f32(const float *center, int64_t center_bstride, const float *lo_map, int64_t lo_bstride,
                                    const float *hi_map, int64_t hi_bstride, const float *target, int64_t target_bstride,
                                    const float *grid, int G, float floor, int *ws, int64_t *hist, int B, int64_t n, void *stream) {
    FD_REQUIRE(center && lo_map && hi_map && target && grid && ws && hist, "fd_interval_hist_f32: null pointer");
    FD_REQUIRE(B > 0 && B <= 65535 && G >= 1 && G <= IV_GMAX && iv_shape_ok(n) && iv_strides_ok(center_bstride, lo_bstride, hi_bstride) &&
                   target_bstride >= 0,
               "fd_interval_hist_f32: unsupported shape B=%d G=%d n=%lld strides %lld %lld %lld %lld", B, G, (long long)n,
               (long long)center_bstride, (long long)lo_bstride, (long long)hi_bstride, (long long)target_bstride);
    FD_REQUIRE(floor > 0.f && floor < INFINITY, "fd_interval_hist_f32: floor must be positive and finite (got %g)", (double)floor);
    const hipStream_t st = (hipStream_t)stream;
    const int nchunk = (int)iv_nchunk(n), P = fd_interval_hist_nblk(n);
    int P2 = 1;
    while (2 * P2 <= G) P2 *= 2;
    const bool vec = n % 4 == 0 && al16(center) && al16(lo_map) && al16(hi_map) && al16(target) && center_bstride % 4 == 0 &&
                     lo_bstride % 4 == 0 && hi_bstride % 4 == 0 && target_bstride % 4 == 0;
    const dim3 grd((unsigned)P, (unsigned)B);
    if (vec)
        hipLaunchKernelGGL(interval_hist_kernel<true>, grd, dim3(256), 0, st, center, center_bstride, lo_map, lo_bstride, hi_map,
                           hi_bstride, target, target_bstride, grid, G, P2, floor, ws, nchunk, n);
    else
        hipLaunchKernelGGL(interval_hist_kernel<false>, grd, dim3(256), 0, st, center, center_bstride, lo_map, lo_bstride, hi_map,
                           hi_bstride, target, target_bstride, grid, G, P2, floor, ws, nchunk, n);
    hipLaunchKernelGGL(interval_hist_finish_kernel, dim3((unsigned)((G + 1 + 255) / 256), (unsigned)B), dim3(256), 0, st, ws, P, G + 1,
                       hist);
    FD_LAUNCH_OK("fd_interval_hist_f32");
    return FD_OK;
}

// floats of workspace per slice of fd_interval_scale_f32: its chunk sums
extern "C" int fd_interval_scale_nblk(int64_t n) { return iv_shape_ok(n) ? (int)iv_nchunk(n) : 0; }

extern "C" int fd_interval_scale_f32(const float *center, int64_t center_bstride, const float *lo_map, int64_t lo_bstride,
                                     const float *hi_map, int64_t hi_bstride, float scale, float floor, float *lo_out, float *hi_out,
                                     float *ws, float *width, int B, int64_t n, void *stream) {
    FD_REQUIRE(center && lo_map && hi_map && lo_out && hi_out && ws && width, "fd_interval_scale_f32: null pointer");
    FD_REQUIRE(B > 0 && B <= 65535 && iv_shape_ok(n) && iv_strides_ok(center_bstride, lo_bstride, hi_bstride),
               "fd_interval_scale_f32: unsupported shape B=%d n=%lld strides %lld %lld %lld", B, (long long)n,
               (long long)center_bstride, (long long)lo_bstride, (long long)hi_bstride);
    FD_REQUIRE(floor > 0.f && floor < INFINITY && scale >= 0.f && scale < INFINITY,
               "fd_interval_scale_f32: floor must be positive, scale non-negative, both finite (got floor=%g scale=%g)", (double)floor,
               (double)scale);
    const hipStream_t st = (hipStream_t)stream;
    const int nchunk = (int)iv_nchunk(n);
    const bool vec = n % 4 == 0 && al16(center) && al16(lo_map) && al16(hi_map) && al16(lo_out) && al16(hi_out) &&
                     center_bstride % 4 == 0 && lo_bstride % 4 == 0 && hi_bstride % 4 == 0;
    const dim3 grd((unsigned)nchunk, (unsigned)B);
    if (vec)
        hipLaunchKernelGGL(interval_scale_kernel<true>, grd, dim3(256), 0, st, center, center_bstride, lo_map, lo_bstride, hi_map,
                           hi_bstride, scale, floor, lo_out, hi_out, ws, nchunk, n);
    else
        hipLaunchKernelGGL(interval_scale_kernel<false>, grd, dim3(256), 0, st, center, center_bstride, lo_map, lo_bstride, hi_map,
                           hi_bstride, scale, floor, lo_out, hi_out, ws, nchunk, n);
    hipLaunchKernelGGL(interval_width_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, ws, nchunk, B, 1.0 / (double)n,
                       width);
    FD_LAUNCH_OK("fd_interval_scale_f32");
    return FD_OK;
}
