// fd_ensemble_orient.hip -- the two transforms around the samplers of an orientation ensemble (ResidualDiffusion.sample_ensemble(
// orientations=...); the reference has no counterpart), and the row gather its conditioning rows need.  fp32, the same code in both
// builds of the library.
//
//   fd_rows_orient_f32            dst[b K + k] = src[b] under the flip / rot90 code codes[k]: fd_rows_repeat_f32 and the orientation in
//                                 one launch.  A copy.
//   fd_ensemble_orient_stats_f32  samples [B][K][H W], replica k read through inv_codes[k], to mean, std, spread and (where asked
//                                 for) the K un-oriented images: the bits of un-orienting every replica and fd_ensemble_stats_f32.
//   fd_rows_take_f32              dst[r] = src[idx[r]]: replicas that share an orientation share a conditioning row.
//
// The code is train_augment's (fd_train_batch.h: src_map / src_offset): bit 0 flips H, bit 1 flips W, bits 2-3 = k.  One workgroup
// owns a 64 x 64 OUTPUT tile and walks the K replicas; a lane owns four groups of four consecutive pixels of a row (orient_tile):
//   direct (k even)  the four source pixels are consecutive: one 16-byte read, reversed in registers under a W flip
//   tiled (k odd)    the source tile is read along ITS rows (16 bytes per lane, 256 bytes per 8 lanes) into float[64][65] in the
//                    LDS and read back along its columns, fd_train_data.hip's form: with the 65-dword pitch the 32 lanes of a half
//                    wave fall into 32 banks on both sides
//   scalar           W % 4 != 0 (H == W where a code transposes, so H % 4 too) or a pointer off 16 bytes: the same ownership, pixel
//                    by pixel, no LDS
// A code is the same for the whole workgroup (it belongs to k), so the form is chosen per replica without divergence.
//
// The statistics are fd_ensemble.hip's, statement for statement: s += x in k order, mean = s / K, q = fmaf(d, d, q) in k order,
// var = q / (K - 1), and they are per pixel, so they do not care which lane owns a pixel.  The spread does: fd_ensemble_stats_f32
// sums var over a lane's four FLAT pixels, then over the 256 lanes of a chunk of 1024 flat pixels.  A 64 x 64 tile holds no whole
// chunk, so the tile kernel leaves var (not std) in the std buffer, and a second kernel with fd_ensemble_stats_f32's lanes reads it
// back (L2), sums it in that order and overwrites it with sqrtf(var): one more read and write of B n floats beside the 2 K n reads,
// for a kernel that reads every source row in 256-byte runs.  The second pass over k re-reads the tile's K sources from L2, as
// fd_ensemble.hip does: no array indexed by k, no cap on K.  No atomics.
#include <vector>
#include "fd_train_batch.h"

namespace {

constexpr int EO_CHUNK = 1024;         // fd_ensemble.hip's ES_CHUNK
constexpr int EO_G = 32;               // and its ES_G
constexpr int EO_LDS = TD_TILE * TD_PITCH;

// The lane's 4 x 4 pixels of the 64 x 64 output tile at (y0, x0) of img under m: v[p] = output pixels (y0 + r + 32 (p >> 1),
// x0 + 4 c + 32 (p & 1) ... + 3), c = tid & 7, r = tid >> 3; 0 outside the image.  m is the same for every lane.
template <bool VEC>
__device__ __forceinline__ void orient_tile(const float *__restrict__ img, const SrcMap m, int y0, int x0, int H, int W, float *lds,
                                            float v[4][4]) {
    const int tid = threadIdx.x, c = tid & 7, r = tid >> 3;
    if (VEC && m.tr) {
        __syncthreads();                                                 // the previous replica's reads of the LDS are done
        // output pixels (y0 + ly4 ... + 3, x0 + lx) have consecutive sources: one 16-byte read, to lds[lx][ly4 ...]
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int lx = r + 32 * (p >> 1), ly4 = 4 * c + 32 * (p & 1);
            const int x = x0 + lx, y = y0 + ly4;
            if (x < W && y < H) {
                const f32x4 q = *(const f32x4 *)(img + src_offset(m, m.fj ? y + 3 : y, x, H, W));
                float *d = lds + lx * TD_PITCH + ly4;
#pragma unroll
                for (int e = 0; e < 4; ++e) d[m.fj ? 3 - e : e] = q[e];
            }
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int lx4 = 4 * c + 32 * (p & 1), ly = r + 32 * (p >> 1);
            const bool in = x0 + lx4 < W && y0 + ly < H;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[p][e] = in ? lds[(lx4 + e) * TD_PITCH + ly] : 0.f;
        }
        return;
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int x = x0 + 4 * c + 32 * (p & 1), y = y0 + r + 32 * (p >> 1);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[p][e] = 0.f;
        if (y >= H || x >= W) continue;
        if (VEC) {
            load4<true>(img + src_offset(m, y, m.fj ? x + 3 : x, H, W), 4, v[p]);
            if (m.fj) {
                float s;
                s = v[p][0]; v[p][0] = v[p][3]; v[p][3] = s;
                s = v[p][1]; v[p][1] = v[p][2]; v[p][2] = s;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (x + e < W) v[p][e] = img[src_offset(m, y, x + e, H, W)];
        }
    }
}

// v[p] to the lane's pixels of the tile at (y0, x0) of out (orient_tile's ownership)
template <bool VEC>
__device__ __forceinline__ void tile_store(float *__restrict__ out, int y0, int x0, int H, int W, const float v[4][4]) {
    const int tid = threadIdx.x, c = tid & 7, r = tid >> 3;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int x = x0 + 4 * c + 32 * (p & 1), y = y0 + r + 32 * (p >> 1);
        if (y < H && x < W) store4<VEC>(out + (int64_t)y * W + x, min(4, W - x), v[p]);
    }
}

// grid (64 x 64 tiles, b)
template <bool VEC>
__global__ __launch_bounds__(256) void rows_orient_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                                         const int *__restrict__ codes, int K, int H, int W, int tiles_x) {
    __shared__ float lds[VEC ? EO_LDS : 1];
    const int b = blockIdx.y, ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    const int y0 = ty * TD_TILE, x0 = tx * TD_TILE;
    const int64_t n = (int64_t)H * W;
    float v[4][4];
    for (int k = 0; k < K; ++k) {
        orient_tile<VEC>(src + (int64_t)b * n, src_map(codes[k] & 15, H == W), y0, x0, H, W, lds, v);
        tile_store<VEC>(dst + ((int64_t)b * K + k) * n, y0, x0, H, W, v);
    }
}

// grid (64 x 64 tiles, b): mean and VAR (in sd) of the tile's pixels, the K un-oriented images where samples_out is given
template <bool VEC>
__global__ __launch_bounds__(256) void orient_stats_kernel(const float *__restrict__ x, const int *__restrict__ inv_codes,
                                                          float *__restrict__ mean, float *__restrict__ sd,
                                                          float *__restrict__ samples_out, int K, int H, int W, int tiles_x) {
    __shared__ float lds[VEC ? EO_LDS : 1];
    const int b = blockIdx.y, ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    const int y0 = ty * TD_TILE, x0 = tx * TD_TILE;
    const bool square = H == W;
    const int64_t n = (int64_t)H * W;
    const float *xp = x + (int64_t)b * K * n;
    float s[4][4], v[4][4], q[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int e = 0; e < 4; ++e) s[p][e] = q[p][e] = 0.f;
    for (int k = 0; k < K; ++k) {
        orient_tile<VEC>(xp + (int64_t)k * n, src_map(inv_codes[k] & 15, square), y0, x0, H, W, lds, v);
        if (samples_out) tile_store<VEC>(samples_out + ((int64_t)b * K + k) * n, y0, x0, H, W, v);
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int e = 0; e < 4; ++e) s[p][e] += v[p][e];
    }
    const float fk = (float)K;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int e = 0; e < 4; ++e) s[p][e] = s[p][e] / fk;              // the mean from here on
    for (int k = 0; k < K; ++k) {
        orient_tile<VEC>(xp + (int64_t)k * n, src_map(inv_codes[k] & 15, square), y0, x0, H, W, lds, v);
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = v[p][e] - s[p][e];
                q[p][e] = fmaf(d, d, q[p][e]);
            }
    }
    const float fk1 = (float)(K - 1);
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int e = 0; e < 4; ++e) q[p][e] = K > 1 ? q[p][e] / fk1 : 0.f;
    tile_store<VEC>(mean + (int64_t)b * n, y0, x0, H, W, s);
    tile_store<VEC>(sd + (int64_t)b * n, y0, x0, H, W, q);
}

// grid (chunk of EO_CHUNK pixels, b), fd_ensemble.hip's lanes: sd holds var; part[b][chunk] = the chunk's sum of var, sd = sqrt(var)
template <bool VEC>
__global__ __launch_bounds__(256) void orient_std_kernel(float *__restrict__ sd, float *__restrict__ part, int64_t part_bstride,
                                                        int64_t n) {
    __shared__ float red[256];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int64_t i0 = (int64_t)blockIdx.x * EO_CHUNK + 4 * tid;
    float acc = 0.f;
    if (i0 < n) {
        const int m = (int)min((int64_t)4, n - i0);
        float var[4], o[4];
        load4<VEC>(sd + (int64_t)b * n + i0, m, var);                    // 0 past the end
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[e] = sqrtf(var[e]);
            acc += var[e];
        }
        store4<VEC>(sd + (int64_t)b * n + i0, m, o);
    }
    const float t = block_sum256(acc, red);
    if (tid == 0) part[(int64_t)b * part_bstride + blockIdx.x] = t;
}

// grid (b / 256), one lane per slice: fd_ensemble.hip's ensemble_finish_kernel
__global__ __launch_bounds__(256) void orient_finish_kernel(const float *__restrict__ stage, int64_t stage_bstride, int M, int B,
                                                           double inv_n, float *__restrict__ spread) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const float *s = stage + (int64_t)b * stage_bstride;
    double t = 0.0;
    for (int m = 0; m < M; ++m) t += (double)s[m];
    spread[b] = (float)sqrt(t * inv_n);
}

// grid (block of 256 vectors, r in steps of gridDim.y)
template <bool VEC>
__global__ __launch_bounds__(256) void rows_take_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                                       const int *__restrict__ idx, int R, int64_t n) {
    const int64_t i0 = 4 * ((int64_t)blockIdx.x * 256 + threadIdx.x);
    if (i0 >= n) return;
    const int m = (int)min((int64_t)4, n - i0);
    for (int r = blockIdx.y; r < R; r += gridDim.y) {
        float v[4];
        load4<VEC>(src + (int64_t)idx[r] * n + i0, m, v);
        store4<VEC>(dst + (int64_t)r * n + i0, m, v);
    }
}

bool eo_shape_ok(int B, int K, int H, int W) {
    return B > 0 && B <= 65535 && K > 0 && K <= 65535 && H > 0 && H <= 32768 && W > 0 && W <= 32768;
}

}  // namespace

extern "C" int fd_rows_orient_f32(const float *src, float *dst, const int *codes, int B, int K, int H, int W, void *stream) {
    FD_REQUIRE(src && dst && codes, "fd_rows_orient_f32: null pointer");
    FD_REQUIRE(eo_shape_ok(B, K, H, W), "fd_rows_orient_f32: unsupported shape B=%d K=%d H=%d W=%d (B, K <= 65535, H, W <= 32768)", B, K,
               H, W);
    const hipStream_t st = (hipStream_t)stream;
    // the codes are the caller's word on what every replica sees: read them back (K ints, once per call, outside any captured loop)
    // so that a code the slice cannot take is an error here and not a quietly different orientation
    std::vector<int> host((size_t)K);
    if (hipMemcpyAsync(host.data(), codes, sizeof(int) * (size_t)K, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        (void)hipGetLastError();
        FD_REQUIRE(false, "fd_rows_orient_f32: codes cannot be read (a device int32 [K] is expected)");
    }
    for (int k = 0; k < K; ++k) {
        FD_REQUIRE(host[k] >= 0 && host[k] <= 15, "fd_rows_orient_f32: code %d of replica %d is outside 0..15", host[k], k);
        FD_REQUIRE(H == W || !(host[k] & 4), "fd_rows_orient_f32: code %d of replica %d transposes, the slice is %d x %d", host[k], k, H,
                   W);
    }
    const int tiles_x = (W + TD_TILE - 1) / TD_TILE, tiles_y = (H + TD_TILE - 1) / TD_TILE;
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)B);
    if (W % 4 == 0 && al16(src) && al16(dst))
        hipLaunchKernelGGL(rows_orient_kernel<true>, grid, dim3(256), 0, st, src, dst, codes, K, H, W, tiles_x);
    else hipLaunchKernelGGL(rows_orient_kernel<false>, grid, dim3(256), 0, st, src, dst, codes, K, H, W, tiles_x);
    FD_LAUNCH_OK("fd_rows_orient_f32");
    return FD_OK;
}

extern "C" int fd_ensemble_orient_stats_f32(const float *samples, const int *inv_codes, float *mean, float *std, float *ws,
                                            float *spread, float *samples_out, int B, int K, int H, int W, void *stream) {
    FD_REQUIRE(samples && inv_codes && mean && std && ws && spread, "fd_ensemble_orient_stats_f32: null pointer");
    FD_REQUIRE(eo_shape_ok(B, K, H, W),
               "fd_ensemble_orient_stats_f32: unsupported shape B=%d K=%d H=%d W=%d (B, K <= 65535, H, W <= 32768)", B, K, H, W);
    const hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)H * W;
    const int nchunk = (int)((n + EO_CHUNK - 1) / EO_CHUNK), M1 = (nchunk + EO_G - 1) / EO_G;
    const int64_t nblk = nchunk + M1;                                    // fd_ensemble_nblk(n)
    float *part = ws, *stage = ws + nchunk;                              // per slice: [nchunk partials][M1 staged sums]
    const int tiles_x = (W + TD_TILE - 1) / TD_TILE, tiles_y = (H + TD_TILE - 1) / TD_TILE;
    const bool vec = W % 4 == 0 && al16(samples) && al16(mean) && al16(std) && (!samples_out || al16(samples_out));
    const dim3 tiles((unsigned)(tiles_x * tiles_y), (unsigned)B), chunks((unsigned)nchunk, (unsigned)B);
    if (vec) {
        hipLaunchKernelGGL(orient_stats_kernel<true>, tiles, dim3(256), 0, st, samples, inv_codes, mean, std, samples_out, K, H, W,
                           tiles_x);
        hipLaunchKernelGGL(orient_std_kernel<true>, chunks, dim3(256), 0, st, std, part, nblk, n);
    } else {
        hipLaunchKernelGGL(orient_stats_kernel<false>, tiles, dim3(256), 0, st, samples, inv_codes, mean, std, samples_out, K, H, W,
                           tiles_x);
        hipLaunchKernelGGL(orient_std_kernel<false>, chunks, dim3(256), 0, st, std, part, nblk, n);
    }
    launch_sum(part, 1, nblk, nchunk, 1, EO_G, stage, 1, nblk, B, st);
    hipLaunchKernelGGL(orient_finish_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, stage, nblk, M1, B,
                       1.0 / (double)n, spread);
    FD_LAUNCH_OK("fd_ensemble_orient_stats_f32");
    return FD_OK;
}

extern "C" int fd_rows_take_f32(const float *src, float *dst, const int *idx, int R, int64_t n, void *stream) {
    FD_REQUIRE(src && dst && idx, "fd_rows_take_f32: null pointer");
    FD_REQUIRE(R > 0 && n > 0 && n < (1ll << 40), "fd_rows_take_f32: unsupported shape R=%d n=%lld", R, (long long)n);
    const dim3 grid((unsigned)cdiv((n + 3) / 4, 256), (unsigned)min(R, 65535));
    if (n % 4 == 0 && al16(src) && al16(dst))
        hipLaunchKernelGGL(rows_take_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, src, dst, idx, R, n);
    else hipLaunchKernelGGL(rows_take_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, src, dst, idx, R, n);
    FD_LAUNCH_OK("fd_rows_take_f32");
    return FD_OK;
}
