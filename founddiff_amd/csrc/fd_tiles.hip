// fd_tiles.hip -- the cut of a slice into overlapping tiles and the blend of the tiles' images back into one slice
// (ResidualDiffusion.sample_tiled; the reference has no counterpart: it denoises whole slices).  fp32, the same code in both builds
// of the library.  The plan is founddiff_amd/tiling.py's: my x mx tiles of th x tw pixels at the origins ys [my], xs [mx] (int32, in
// device memory, increasing, the last one H - th / W - tw), tile row (b my + iy) mx + ix of a slice b.
//
//   fd_tiles_gather_f32  dst[(b my + iy) mx + ix] = the th x tw window of src[b] at (ys[iy], xs[ix]): a copy.  Used for the input
//                        planes and for the x_T field, so that overlapping tiles start from the same noise in their common pixels.
//   fd_tiles_blend_f32   out[b][y][x] = sum w v / sum w over the tiles that cover (y, x), w = wy[iy][y - ys[iy]] wx[ix][x - xs[ix]].
//
// Both are bandwidth kernels: a lane owns 4 consecutive pixels of a row (one 16-byte access where the launch allows it), a wave a
// contiguous stretch of a row.  The blend is a gather: every output pixel is owned by one lane, which walks the tiles in row-major
// tile order (iy ascending, then ix ascending) -- no atomics, no workspace, and a pixel depends on (H, W, the plan, its covering
// tiles) alone, not on B.  Per element the arithmetic is w = wy * wx, num = fmaf(w, v, num), den += w, out = num / den (the
// correctly rounded division: no rcp), the same on the 16-byte path and on the scalar path, so the two give the same bits; a pixel
// under one tile has w = 1 and den = 1 (tiling.tile_weights: a lone tile's weight is exactly 1), so out is that tile's value bit for
// bit.  The row test (iy) is uniform over a wave wherever a wave lies inside one row (W >= 256); the column test (ix) skips a load
// for the lanes outside the tile, it selects no other code.  Origins outside the slice (a plan that is not tile_plan's) are not
// followed: the lanes of such a tile do nothing.
#include "fd_train_common.h"

namespace {

// grid (blocks of 256 lanes over th x ceil(tw / 4) groups, tile row r)
template <bool VEC>
__global__ __launch_bounds__(256) void tiles_gather_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                                          const int *__restrict__ ys, const int *__restrict__ xs, int H, int W,
                                                          int th, int tw, int my, int mx) {
    const int tw4 = (tw + 3) >> 2;
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= th * tw4) return;
    const int r = blockIdx.y;
    const int ix = r % mx, q = r / mx;
    const int iy = q % my, b = q / my;
    const int ya = ys[iy], xa = xs[ix];
    if (ya < 0 || ya > H - th || xa < 0 || xa > W - tw) return;
    const int y = g / tw4, x0 = 4 * (g - y * tw4);
    const int m = min(4, tw - x0);
    float v[4];
    load4<VEC>(src + ((int64_t)b * H + ya + y) * W + xa + x0, m, v);
    store4<VEC>(dst + ((int64_t)r * th + y) * tw + x0, m, v);
}

// grid (blocks of 256 lanes over H x ceil(W / 4) groups, b)
template <bool VEC>
__global__ __launch_bounds__(256) void tiles_blend_kernel(const float *__restrict__ tiles, const float *__restrict__ wy,
                                                         const float *__restrict__ wx, const int *__restrict__ ys,
                                                         const int *__restrict__ xs, float *__restrict__ out, int H, int W, int th,
                                                         int tw, int my, int mx) {
    const int W4 = (W + 3) >> 2;
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= H * W4) return;
    const int b = blockIdx.y;
    const int y = g / W4, x0 = 4 * (g - y * W4);
    const int m = min(4, W - x0);
    float num[4] = {0.f, 0.f, 0.f, 0.f}, den[4] = {0.f, 0.f, 0.f, 0.f};
    for (int iy = 0; iy < my; ++iy) {
        const int ya = ys[iy];
        if (ya < 0 || ya > H - th || y < ya || y >= ya + th) continue;
        const float fy = wy[iy * th + (y - ya)];
        const float *trow = tiles + (((int64_t)b * my + iy) * mx * th + (y - ya)) * tw;      // row y - ya of tile (b, iy, 0)
        for (int ix = 0; ix < mx; ++ix) {
            const int xa = xs[ix];
            if (xa < 0 || xa > W - tw || x0 + m <= xa || x0 >= xa + tw) continue;
            const int u0 = x0 - xa;                                      // local column of element 0: may be negative on the scalar path
            const float *tp = trow + (int64_t)ix * th * tw + u0;
            const float *wp = wx + ix * tw + u0;
            if (VEC) {                                                   // xs, tw multiples of 4: the group lies inside the tile
                float v[4], fx[4];
                load4<true>(tp, 4, v);
                load4<true>(wp, 4, fx);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float w = fy * fx[e];
                    num[e] = fmaf(w, v[e], num[e]);
                    den[e] += w;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (e < m && u0 + e >= 0 && u0 + e < tw) {
                        const float w = fy * wp[e];
                        num[e] = fmaf(w, tp[e], num[e]);
                        den[e] += w;
                    }
                }
            }
        }
    }
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = num[e] / den[e];                   // an uncovered pixel (no plan of tile_plan has one): 0 / 0
    store4<VEC>(out + ((int64_t)b * H + y) * W + x0, m, o);
}

bool tiles_shape_ok(int B, int H, int W, int th, int tw, int my, int mx) {
    return B > 0 && H > 0 && W > 0 && H <= 32768 && W <= 32768 && th >= 1 && th <= H && tw >= 1 && tw <= W && my >= 1 && mx >= 1 &&
           (int64_t)B * my * mx <= 65535;
}

}  // namespace

extern "C" int fd_tiles_gather_f32(const float *src, float *dst, const int *ys, const int *xs, int B, int H, int W, int th, int tw,
                                   int my, int mx, int xs_mult4, void *stream) {
    FD_REQUIRE(src && dst && ys && xs, "fd_tiles_gather_f32: null pointer");
    FD_REQUIRE(tiles_shape_ok(B, H, W, th, tw, my, mx),
               "fd_tiles_gather_f32: unsupported shape B=%d H=%d W=%d th=%d tw=%d my=%d mx=%d (1 <= th <= H, 1 <= tw <= W, my, mx >= 1, "
               "B my mx <= 65535, H, W <= 32768)", B, H, W, th, tw, my, mx);
    const bool vec = xs_mult4 && W % 4 == 0 && tw % 4 == 0 && al16(src) && al16(dst);
    const dim3 grid((unsigned)cdiv((int64_t)th * ((tw + 3) / 4), 256), (unsigned)(B * my * mx));
    if (vec) hipLaunchKernelGGL(tiles_gather_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, src, dst, ys, xs, H, W, th, tw, my, mx);
    else hipLaunchKernelGGL(tiles_gather_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, src, dst, ys, xs, H, W, th, tw, my, mx);
    FD_LAUNCH_OK("fd_tiles_gather_f32");
    return FD_OK;
}

extern "C" int fd_tiles_blend_f32(const float *tiles, const float *wy, const float *wx, const int *ys, const int *xs, float *out,
                                  int B, int H, int W, int th, int tw, int my, int mx, int xs_mult4, void *stream) {
    FD_REQUIRE(tiles && wy && wx && ys && xs && out, "fd_tiles_blend_f32: null pointer");
    FD_REQUIRE(tiles_shape_ok(B, H, W, th, tw, my, mx),
               "fd_tiles_blend_f32: unsupported shape B=%d H=%d W=%d th=%d tw=%d my=%d mx=%d (1 <= th <= H, 1 <= tw <= W, my, mx >= 1, "
               "B my mx <= 65535, H, W <= 32768)", B, H, W, th, tw, my, mx);
    const bool vec = xs_mult4 && W % 4 == 0 && tw % 4 == 0 && al16(tiles) && al16(wx) && al16(out);
    const dim3 grid((unsigned)cdiv((int64_t)H * ((W + 3) / 4), 256), (unsigned)B);
    if (vec) hipLaunchKernelGGL(tiles_blend_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, tiles, wy, wx, ys, xs, out, H, W, th, tw, my, mx);
    else hipLaunchKernelGGL(tiles_blend_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, tiles, wy, wx, ys, xs, out, H, W, th, tw, my, mx);
    FD_LAUNCH_OK("fd_tiles_blend_f32");
    return FD_OK;
}
