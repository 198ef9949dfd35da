// fd_tiles_step.hip -- one sampler step of a slice held as overlapping tiles, the tiles' raw model outputs blended per pixel before
// the update (ResidualDiffusion.sample_tiled(fuse="step"); the reference has no counterpart).  fp32, the same code in both builds of
// the library.  The plan is fd_tiles.hip's: my x mx tiles of th x tw pixels at the origins ys [my], xs [mx], weights wy [my][th],
// wx [mx][tw], tile row r = (b my + iy) mx + ix; o0, o1, x_t, x_in, img_out are [B my mx][th tw] in that order.
//
//   fd_tiles_step_ddim_f32   the DDIM step of fd_res_step_obj (step == 1, no noise), par = {ac, bc, omac, alpha, -, -, -, last}
//   fd_tiles_step_keyed_f32  the ancestral step of fd_res_step_obj_keyed: row *t_dev of the [T][8] table, keyed noise
//
// The lanes are tile-owned: a lane owns 4 consecutive pixels of one tile row (one 16-byte access per stream where the launch
// allows it) and for its pixel (y, x) of slice b
//   blends   every stream the mode reads over the tiles that cover (y, x), in row-major tile order (iy ascending, then ix): w = wy wx,
//            num = fmaf(w, v, num), den += w, o = num / den -- tiles_blend_kernel's arithmetic, so a pixel under one tile takes that
//            tile's output bit for bit;
//   updates  with fd_obj_pixel.h's per-pixel code on the blended outputs, its own x_t and its own x_in -- a one-tile plan is
//            fd_res_step_obj_keyed (fd_res_step_obj step 1), bit for bit;
//   draws    the keyed form's noise at the SLICE pixel: element (y W + x) % 4 of keyed_normal4(slice seed, t, (y W + x) / 4), the
//            field fd_keyed_normal gives for the whole slice, so overlapping tiles receive the same noise;
//   writes   its own img_out pixel (img_out may be x_t: a lane reads its own x_t pixels before it writes them, and reads of other
//            tiles go to o0 / o1 alone, which the kernel never writes), and, where slice_out is given and its tile is the first of
//            the covering tiles in that order, the slice pixel.
// Rows whose x_t and x_in agree in the common pixels of overlapping tiles (gathered from one slice) therefore agree in them after
// the step, and slice_out is every covering tile's value.  No atomics, no workspace, nothing depends on B.  The 16-byte form needs
// xs and tw multiples of 4 and W % 4 == 0: a lane's group is then a noise group of the slice and lies inside or outside a tile as
// a whole.  The scalar form tests every pixel and picks its noise from up to two groups; the arithmetic per pixel is the same.
#include "fd_train_common.h"
#include "fd_keyed_noise.h"
#include "fd_obj_pixel.h"

namespace {

// grid (blocks of 256 lanes over th x ceil(tw / 4) groups, tile row r).  xt / out may be the same buffer: no __restrict__ on them.
template <int MODE, bool KEYED, bool VEC>
__global__ __launch_bounds__(256) void tiles_step_kernel(const float *__restrict__ o0, const float *__restrict__ o1, const float *xt,
                                                        const float *__restrict__ xin, const float *__restrict__ par,
                                                        const int *__restrict__ t_dev, const int64_t *__restrict__ seeds,
                                                        const float *__restrict__ wy, const float *__restrict__ wx,
                                                        const int *__restrict__ ys, const int *__restrict__ xs, float *out,
                                                        float *__restrict__ slice_out, int H, int W, int th, int tw, int my, int mx,
                                                        int T) {
    constexpr bool R0 = MODE != 1, R1 = MODE == 1 || MODE == 2, RI = MODE != 2;
    const int tw4 = (tw + 3) >> 2;
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= th * tw4) return;
    const int r = blockIdx.y;
    const int ixo = r % mx, q = r / mx;
    const int iyo = q % my, b = q / my;
    const int yo = ys[iyo], xo = xs[ixo];
    if (yo < 0 || yo > H - th || xo < 0 || xo > W - tw) return;
    const int yl = g / tw4, u = 4 * (g - yl * tw4);
    const int m = min(4, tw - u);
    const int y = yo + yl, x0 = xo + u;                                   // the group's first pixel in the slice

    // ---- blend the streams over the covering tiles; seen / mine: bit e = pixel e is covered / this tile is its first cover
    float n0[4] = {0.f, 0.f, 0.f, 0.f}, n1[4] = {0.f, 0.f, 0.f, 0.f}, den[4] = {0.f, 0.f, 0.f, 0.f};
    int seen = 0, mine = 0;
    for (int iy = 0; iy < my; ++iy) {
        const int ya = ys[iy];
        if (ya < 0 || ya > H - th || y < ya || y >= ya + th) continue;
        const float fy = wy[iy * th + (y - ya)];
        const int64_t trow = (((int64_t)b * my + iy) * mx * th + (y - ya)) * tw;     // row y - ya of tile (b, iy, 0)
        for (int ix = 0; ix < mx; ++ix) {
            const int xa = xs[ix];
            if (xa < 0 || xa > W - tw || x0 + m <= xa || x0 >= xa + tw) continue;
            const int u0 = x0 - xa;                                      // local column of pixel 0: may be negative on the scalar path
            const int64_t tp = trow + (int64_t)ix * th * tw + u0;
            const float *wp = wx + ix * tw + u0;
            const int own = (iy == iyo && ix == ixo) ? 15 : 0;
            if (VEC) {                                                   // xs, tw multiples of 4: the group lies inside the tile
                float v0[4], v1[4], fx[4];
                load4<true>(wp, 4, fx);
                if (R0) load4<true>(o0 + tp, 4, v0);
                if (R1) load4<true>(o1 + tp, 4, v1);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float w = fy * fx[e];
                    if (R0) n0[e] = fmaf(w, v0[e], n0[e]);
                    if (R1) n1[e] = fmaf(w, v1[e], n1[e]);
                    den[e] += w;
                }
                mine |= own & ~seen;
                seen = 15;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (e < m && u0 + e >= 0 && u0 + e < tw) {
                        const float w = fy * wp[e];
                        if (R0) n0[e] = fmaf(w, o0[tp + e], n0[e]);
                        if (R1) n1[e] = fmaf(w, o1[tp + e], n1[e]);
                        den[e] += w;
                        mine |= own & ~seen & (1 << e);
                        seen |= 1 << e;
                    }
                }
            }
        }
    }

    // ---- the step's parameters and noise
    float pa = 0.f, pb = 0.f, poma = 0.f, alpha = 0.f;
    bool last = false;
    obj_row row = {};
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (KEYED) {
        const int t = min(max(*t_dev, 0), T - 1);
        const float *p = par + (int64_t)t * 8;
        row.a = p[0]; row.bb = p[1]; row.oma = p[2]; row.c1 = p[3]; row.c2 = p[4]; row.c3 = p[5];
        row.sd = t > 0 ? expf(0.5f * p[6]) : 0.f;                        // no noise at t = 0 (src/DADiff.py:1228)
        if (t > 0) {
            const uint64_t seed = (uint64_t)seeds[b];
            const int64_t p0 = (int64_t)y * W + x0;                      // < 2^30: H, W <= 32768
            if (VEC) {
                keyed_normal4(seed, (uint32_t)t, (uint32_t)(p0 >> 2), z);
            } else {
                const int sh = (int)(p0 & 3);
                float za[4], zb[4] = {0.f, 0.f, 0.f, 0.f};
                keyed_normal4(seed, (uint32_t)t, (uint32_t)(p0 >> 2), za);
                if (sh + m > 4) keyed_normal4(seed, (uint32_t)t, (uint32_t)(p0 >> 2) + 1u, zb);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (k == sh + e) z[e] = k < 4 ? za[k & 3] : zb[k & 3];
            }
        }
    } else {
        pa = par[0]; pb = par[1]; poma = par[2]; alpha = par[3];
        last = par[7] != 0.f;
    }

    // ---- update the lane's own pixels
    const int64_t j = ((int64_t)r * th + yl) * tw + u;
    float vx[4], vi[4] = {0.f, 0.f, 0.f, 0.f}, res[4];
    load4<VEC>(xt + j, m, vx);
    if (RI) load4<VEC>(xin + j, m, vi);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float b0 = R0 ? n0[e] / den[e] : 0.f, b1 = R1 ? n1[e] / den[e] : 0.f;      // lanes past the row's end: 0 / 0, not stored
        res[e] = KEYED ? obj_pixel<MODE>(row, b0, b1, vx[e], vi[e], z[e])
                       : obj_ddim_pixel<MODE>(pa, pb, poma, alpha, last, b0, b1, vx[e], vi[e]);
    }
    store4<VEC>(out + j, m, res);
    if (slice_out) {
        float *sp = slice_out + ((int64_t)b * H + y) * W + x0;
        if (VEC) {
            if (mine) store4<true>(sp, 4, res);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < m && (mine >> e & 1)) sp[e] = res[e];
        }
    }
}

bool tiles_shape_ok(int B, int H, int W, int th, int tw, int my, int mx) {
    return B > 0 && H > 0 && W > 0 && H <= 32768 && W <= 32768 && th >= 1 && th <= H && tw >= 1 && tw <= W && my >= 1 && mx >= 1 &&
           (int64_t)B * my * mx <= 65535;
}

struct step_args {
    const float *o0, *o1, *x_t, *x_in, *par;
    const int *t_dev;
    const int64_t *seeds;
    const float *wy, *wx;
    const int *ys, *xs;
    float *img_out, *slice_out;
    int B, H, W, th, tw, my, mx, xs_mult4, T;
};

template <int MODE, bool KEYED>
void launch_step(const step_args &a, hipStream_t s) {
    const bool vec = a.xs_mult4 && a.W % 4 == 0 && a.tw % 4 == 0 && al16(a.x_t) && al16(a.img_out) && al16(a.wx) &&
                     (MODE == 1 || al16(a.o0)) && ((MODE != 1 && MODE != 2) || al16(a.o1)) && (MODE == 2 || al16(a.x_in)) &&
                     al16(a.slice_out);
    const dim3 grid((unsigned)cdiv((int64_t)a.th * ((a.tw + 3) / 4), 256), (unsigned)(a.B * a.my * a.mx));
    if (vec)
        hipLaunchKernelGGL((tiles_step_kernel<MODE, KEYED, true>), grid, dim3(256), 0, s, a.o0, a.o1, a.x_t, a.x_in, a.par, a.t_dev,
                           a.seeds, a.wy, a.wx, a.ys, a.xs, a.img_out, a.slice_out, a.H, a.W, a.th, a.tw, a.my, a.mx, a.T);
    else
        hipLaunchKernelGGL((tiles_step_kernel<MODE, KEYED, false>), grid, dim3(256), 0, s, a.o0, a.o1, a.x_t, a.x_in, a.par, a.t_dev,
                           a.seeds, a.wy, a.wx, a.ys, a.xs, a.img_out, a.slice_out, a.H, a.W, a.th, a.tw, a.my, a.mx, a.T);
}

template <bool KEYED>
void launch_mode(int mode, const step_args &a, hipStream_t s) {
    if (mode == 0) launch_step<0, KEYED>(a, s);
    else if (mode == 1) launch_step<1, KEYED>(a, s);
    else if (mode == 2) launch_step<2, KEYED>(a, s);
    else launch_step<3, KEYED>(a, s);
}

// what both entry points ask of their arguments: the streams the mode reads, and fd_tiles.hip's shape limits
int step_checks(const char *fn, int mode, const step_args &a) {
    FD_REQUIRE(mode >= 0 && mode <= 3, "%s: bad mode %d", fn, mode);
    FD_REQUIRE(a.x_t && a.par && a.wy && a.wx && a.ys && a.xs && a.img_out, "%s: null pointer", fn);
    FD_REQUIRE((mode == 1 || a.o0) && ((mode != 1 && mode != 2) || a.o1) && (mode == 2 || a.x_in), "%s: mode %d needs o0=%p o1=%p x_in=%p",
               fn, mode, (const void *)a.o0, (const void *)a.o1, (const void *)a.x_in);
    FD_REQUIRE(tiles_shape_ok(a.B, a.H, a.W, a.th, a.tw, a.my, a.mx),
               "%s: unsupported shape B=%d H=%d W=%d th=%d tw=%d my=%d mx=%d (1 <= th <= H, 1 <= tw <= W, my, mx >= 1, "
               "B my mx <= 65535, H, W <= 32768)", fn, a.B, a.H, a.W, a.th, a.tw, a.my, a.mx);
    return FD_OK;
}

}  // namespace

extern "C" int fd_tiles_step_ddim_f32(int mode, const float *o0, const float *o1, const float *x_t, const float *x_in,
                                      const float *par, const float *wy, const float *wx, const int *ys, const int *xs, int B, int H,
                                      int W, int th, int tw, int my, int mx, int xs_mult4, float *img_out, float *slice_out,
                                      void *stream) {
    const step_args a = {o0, o1, x_t, x_in, par, nullptr, nullptr, wy, wx, ys, xs, img_out, slice_out, B, H, W, th, tw, my, mx, xs_mult4, 1};
    if (const int e = step_checks("fd_tiles_step_ddim_f32", mode, a)) return e;
    launch_mode<false>(mode, a, (hipStream_t)stream);
    FD_LAUNCH_OK("fd_tiles_step_ddim_f32");
    return FD_OK;
}

extern "C" int fd_tiles_step_keyed_f32(int mode, const float *o0, const float *o1, const float *x_t, const float *x_in,
                                       const float *par_table, const int *t_dev, const int64_t *slice_seeds, const float *wy,
                                       const float *wx, const int *ys, const int *xs, int B, int H, int W, int th, int tw, int my,
                                       int mx, int xs_mult4, float *img_out, float *slice_out, int T, void *stream) {
    const step_args a = {o0, o1, x_t, x_in, par_table, t_dev, slice_seeds, wy, wx, ys, xs, img_out, slice_out, B, H, W, th, tw, my, mx,
                         xs_mult4, T};
    if (const int e = step_checks("fd_tiles_step_keyed_f32", mode, a)) return e;
    FD_REQUIRE(t_dev && slice_seeds, "fd_tiles_step_keyed_f32: null pointer");
    FD_REQUIRE(T > 0, "fd_tiles_step_keyed_f32: bad table size T=%d", T);
    launch_mode<true>(mode, a, (hipStream_t)stream);
    FD_LAUNCH_OK("fd_tiles_step_keyed_f32");
    return FD_OK;
}
