// fd_tiles_ensemble.hip -- the final tile images of K keyed realisations per slice, straight to the ensemble's statistics
// (ResidualDiffusion.sample_ensemble(tile=...), fuse "final"; the reference has no counterpart).  fp32, the same code in both builds
// of the library.
//
//   fd_tiles_ensemble_f32  tiles [B K my mx][th tw] (row ((b K + k) my + iy) mx + ix) -> mean, std [B][H W], spread [B], and the K
//                          blended slice images samples [B K][H W] where the caller gives a pointer for them.
//
// The specification is bitwise: fd_tiles_blend_f32 over the B K pseudo-slices followed by fd_ensemble_stats_f32(B, K, H W), so the
// arithmetic of both files is restated here, statement for statement (the compiler must meet the same expressions to make the same
// contraction decisions: `den += w` below is written as fd_tiles.hip writes it).  The lanes are fd_ensemble_stats_f32's: grid
// (chunk of 1024 flat pixels, b), a lane owns four consecutive FLAT pixels, so a chunk's partial of the spread is the same sum.  On
// the 16-byte form (W % 4 == 0, origins and tw multiples of 4) the four pixels lie in one row and inside or outside a tile
// together; on the scalar form they may straddle two rows and every pixel finds its tiles on its own.
// Two passes over k, as in fd_ensemble.hip.  The second one blends AGAIN from the tiles instead of holding K blended values: the
// covering tiles of a workgroup's 1024 pixels are K x (at most a few) x 4 KB that it has just pulled into L2, it costs a second
// division per replica and pixel on a kernel that waits for memory, and it leaves the kernel without a cap on K and without a
// register array indexed by k (which would be scratch for any K the compiler cannot see).  Within a pass the replicas go TE_KB at
// a time through one walk of the plan, so that a lane has TE_KB tile loads in flight.  No atomics, no LDS beyond the block sum.
#include "fd_train_common.h"

namespace {

constexpr int TE_CHUNK = 1024;         // fd_ensemble.hip's ES_CHUNK: pixels of a slice per workgroup
constexpr int TE_G = 32;               // and its ES_G: partials per launch_sum group
constexpr int TE_KB = 4;               // replicas blended together (blend_row4): a bound on registers, not on K

struct TePlan {
    const float *wy, *wx;
    const int *ys, *xs;
    int H, W, th, tw, my, mx;
};

// The blends of nk <= TE_KB consecutive replicas at once.  The walk over the plan and the weights are the same for every replica,
// and so is den; the replicas' tile loads do not depend on one another, so TE_KB of them are in flight where one replica at a time
// would wait for each in turn.  Per replica the chain num = fmaf(w, v, num) runs over the covering tiles in the same order.
// tiles: replica 0 of the block, kstride floats per replica.

// four pixels of row y starting at column x0 (16-byte form: the group lies inside or outside a tile as a whole)
__device__ __forceinline__ void blend_row4(const float *__restrict__ tiles, int64_t kstride, int nk, const TePlan &p, int y, int x0,
                                           float o[TE_KB][4]) {
    float num[TE_KB][4], den[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < TE_KB; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) num[j][e] = 0.f;
    for (int iy = 0; iy < p.my; ++iy) {
        const int ya = p.ys[iy];
        if (ya < 0 || ya > p.H - p.th || y < ya || y >= ya + p.th) continue;
        const float fy = p.wy[iy * p.th + (y - ya)];
        const float *trow = tiles + ((int64_t)iy * p.mx * p.th + (y - ya)) * p.tw;              // row y - ya of tile (iy, 0)
        for (int ix = 0; ix < p.mx; ++ix) {
            const int xa = p.xs[ix];
            if (xa < 0 || xa > p.W - p.tw || x0 + 4 <= xa || x0 >= xa + p.tw) continue;
            const int u0 = x0 - xa;
            const float *tp = trow + (int64_t)ix * p.th * p.tw + u0;
            float v[TE_KB][4], fx[4];
#pragma unroll
            for (int j = 0; j < TE_KB; ++j) {
                if (j < nk) load4<true>(tp + j * kstride, 4, v[j]);
                else v[j][0] = v[j][1] = v[j][2] = v[j][3] = 0.f;
            }
            load4<true>(p.wx + ix * p.tw + u0, 4, fx);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float w = fy * fx[e];
#pragma unroll
                for (int j = 0; j < TE_KB; ++j) num[j][e] = fmaf(w, v[j][e], num[j][e]);
                den[e] += w;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < TE_KB; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) o[j][e] = num[j][e] / den[e];
}

// pixel (y, x) alone (scalar form)
__device__ __forceinline__ void blend_px(const float *__restrict__ tiles, int64_t kstride, int nk, const TePlan &p, int y, int x,
                                         float o[TE_KB]) {
    float num[TE_KB], den = 0.f;
#pragma unroll
    for (int j = 0; j < TE_KB; ++j) num[j] = 0.f;
    for (int iy = 0; iy < p.my; ++iy) {
        const int ya = p.ys[iy];
        if (ya < 0 || ya > p.H - p.th || y < ya || y >= ya + p.th) continue;
        const float fy = p.wy[iy * p.th + (y - ya)];
        const float *trow = tiles + ((int64_t)iy * p.mx * p.th + (y - ya)) * p.tw;
        for (int ix = 0; ix < p.mx; ++ix) {
            const int xa = p.xs[ix];
            if (xa < 0 || xa > p.W - p.tw || x < xa || x >= xa + p.tw) continue;
            const float *tp = trow + (int64_t)ix * p.th * p.tw + (x - xa);
            float v[TE_KB];
#pragma unroll
            for (int j = 0; j < TE_KB; ++j) v[j] = j < nk ? tp[j * kstride] : 0.f;
            const float w = fy * p.wx[ix * p.tw + (x - xa)];
#pragma unroll
            for (int j = 0; j < TE_KB; ++j) num[j] = fmaf(w, v[j], num[j]);
            den += w;
        }
    }
#pragma unroll
    for (int j = 0; j < TE_KB; ++j) o[j] = num[j] / den;                 // an uncovered pixel (no plan of tile_plan has one): 0 / 0
}

// the images of nk replicas at the lane's m <= 4 flat pixels from i0 on; elements past the end of the slice are 0, as load4<false>
// reads them; the rows j >= nk are not used
template <bool VEC>
__device__ __forceinline__ void blend4(const float *__restrict__ tiles, int64_t kstride, int nk, const TePlan &p, int i0, int m,
                                       float v[TE_KB][4]) {
    if (VEC) {
        const int y = i0 / p.W;
        blend_row4(tiles, kstride, nk, p, y, i0 - y * p.W, v);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float o[TE_KB];
#pragma unroll
            for (int j = 0; j < TE_KB; ++j) o[j] = 0.f;
            if (e < m) {
                const int y = (i0 + e) / p.W;
                blend_px(tiles, kstride, nk, p, y, i0 + e - y * p.W, o);
            }
#pragma unroll
            for (int j = 0; j < TE_KB; ++j) v[j][e] = o[j];
        }
    }
}

// grid (chunk of TE_CHUNK pixels, b): fd_ensemble.hip's ensemble_stats_kernel with the blend in the place of its loads
template <bool VEC>
__global__ __launch_bounds__(256) void tiles_ensemble_kernel(const float *__restrict__ tiles, TePlan p, float *__restrict__ samples,
                                                            float *__restrict__ mean, float *__restrict__ sd,
                                                            float *__restrict__ part, int64_t part_bstride, int K) {
    __shared__ float red[256];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int n = p.H * p.W;                                             // H, W <= 32768: at most 2^30
    const int i0 = blockIdx.x * TE_CHUNK + 4 * tid;
    float acc = 0.f;
    if (i0 < n) {
        const int m = min(4, n - i0);
        const int64_t kstride = (int64_t)p.my * p.mx * p.th * p.tw;      // floats of one replica's tiles
        const float *tp = tiles + (int64_t)b * K * kstride;
        float s[4] = {0.f, 0.f, 0.f, 0.f}, v[TE_KB][4], mu[4], q[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
        for (int k0 = 0; k0 < K; k0 += TE_KB) {
            const int nk = min(TE_KB, K - k0);
            blend4<VEC>(tp + (int64_t)k0 * kstride, kstride, nk, p, i0, m, v);
#pragma unroll
            for (int j = 0; j < TE_KB; ++j) {
                if (j < nk) {                                            // in k order
                    if (samples) store4<VEC>(samples + ((int64_t)b * K + k0 + j) * n + i0, m, v[j]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) s[e] += v[j][e];
                }
            }
        }
        const float fk = (float)K;
#pragma unroll
        for (int e = 0; e < 4; ++e) mu[e] = s[e] / fk;
        for (int k0 = 0; k0 < K; k0 += TE_KB) {
            const int nk = min(TE_KB, K - k0);
            blend4<VEC>(tp + (int64_t)k0 * kstride, kstride, nk, p, i0, m, v);
#pragma unroll
            for (int j = 0; j < TE_KB; ++j) {
                if (j < nk) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float d = v[j][e] - mu[e];
                        q[e] = fmaf(d, d, q[e]);
                    }
                }
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

// grid (b / 256), one lane per slice: fd_ensemble.hip's ensemble_finish_kernel
__global__ __launch_bounds__(256) void tiles_ensemble_finish_kernel(const float *__restrict__ stage, int64_t stage_bstride, int M,
                                                                   int B, double inv_n, float *__restrict__ spread) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const float *s = stage + (int64_t)b * stage_bstride;
    double t = 0.0;
    for (int m = 0; m < M; ++m) t += (double)s[m];
    spread[b] = (float)sqrt(t * inv_n);
}

}  // namespace

extern "C" int fd_tiles_ensemble_f32(const float *tiles, const float *wy, const float *wx, const int *ys, const int *xs,
                                     float *samples, float *mean, float *std, float *ws, float *spread, int B, int K, int H, int W,
                                     int th, int tw, int my, int mx, int xs_mult4, void *stream) {
    FD_REQUIRE(tiles && wy && wx && ys && xs && mean && std && ws && spread, "fd_tiles_ensemble_f32: null pointer");
    FD_REQUIRE(K >= 1, "fd_tiles_ensemble_f32: K must be at least 1 (got %d)", K);
    FD_REQUIRE(B > 0 && H > 0 && W > 0 && H <= 32768 && W <= 32768 && th >= 1 && th <= H && tw >= 1 && tw <= W && my >= 1 && mx >= 1 &&
                   (int64_t)B * K * my * mx <= 65535,
               "fd_tiles_ensemble_f32: unsupported shape B=%d K=%d H=%d W=%d th=%d tw=%d my=%d mx=%d (1 <= th <= H, 1 <= tw <= W, my, "
               "mx >= 1, B K my mx <= 65535, H, W <= 32768)", B, K, H, W, th, tw, my, mx);
    const hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)H * W;
    const int nchunk = (int)((n + TE_CHUNK - 1) / TE_CHUNK), M1 = (nchunk + TE_G - 1) / TE_G;
    const int64_t nblk = nchunk + M1;                                    // fd_ensemble_nblk(n)
    float *part = ws, *stage = ws + nchunk;                              // per slice: [nchunk partials][M1 staged sums]
    const TePlan p = {wy, wx, ys, xs, H, W, th, tw, my, mx};
    const bool vec = xs_mult4 && W % 4 == 0 && tw % 4 == 0 && al16(tiles) && al16(wx) && al16(mean) && al16(std) &&
                     (!samples || al16(samples));
    const dim3 grid((unsigned)nchunk, (unsigned)B);
    if (vec) hipLaunchKernelGGL(tiles_ensemble_kernel<true>, grid, dim3(256), 0, st, tiles, p, samples, mean, std, part, nblk, K);
    else hipLaunchKernelGGL(tiles_ensemble_kernel<false>, grid, dim3(256), 0, st, tiles, p, samples, mean, std, part, nblk, K);
    launch_sum(part, 1, nblk, nchunk, 1, TE_G, stage, 1, nblk, B, st);
    hipLaunchKernelGGL(tiles_ensemble_finish_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, stage, nblk, M1, B,
                       1.0 / (double)n, spread);
    FD_LAUNCH_OK("fd_tiles_ensemble_f32");
    return FD_OK;
}
