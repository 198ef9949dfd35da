// fd_outer_train.hip -- the two outer convolutions of the U-Net for training (src/DADiff.py:553-555 init_conv, 681 final_conv), the
// last full-resolution activation ops of a step that were torch's:
//
//   fd_init_conv7_fwd_f32    x (B, Cin, H, W) planes, Cin 2 or 3 -> out (B, H, W, Cout) channel-last, 7x7 / padding 3
//   fd_init_conv7_wgrad_f32  dweight and dbias from x and dout in one pass over dout (dout is the only large operand)
//   fd_final_conv1_fwd_f32   x channels [off, off + C) of (npix, ld) -> out (npix), 1x1 to one plane
//   fd_final_conv1_bwd_f32   dx, dweight and dbias in one pass: reads x and dout, writes dx
//
// Exact fp32 (fmaf chains on the VALU: the fp32 MFMA runs at the vector rate and the taps of a 7x7 window on 2-3 planes have no
// channel axis to feed it), no float atomics, no host synchronisation.  An output element's summation order depends on the layer's
// shape alone, so out and dx of a slice do not depend on its batch; the weight gradients are fixed-order partial sums plus a
// reduce (fd_train_common.h).
#include "fd_train_common.h"

namespace {

// ---- init_conv -----------------------------------------------------------------------------------------------------------------
// A tile is IC_TY x IC_TX pixels; its halo of x is (IC_TY + 6) x (IC_TX + 6) per plane, zero outside the image.
constexpr int IC_TX = 32, IC_HX = IC_TX + 6, IC_LDX = 40;                // LDS row stride of the halo
constexpr int IC_MAXC = 3;

struct Tile {
    int b, y0, x0;
};

__device__ __forceinline__ Tile tile_of(int64_t t, int tiles_x, int tiles_y, int TY) {
    Tile r;
    r.x0 = (int)(t % tiles_x) * IC_TX;
    const int64_t q = t / tiles_x;
    r.y0 = (int)(q % tiles_y) * TY;
    r.b = (int)(q / tiles_y);
    return r;
}

// the halo of tile t of every plane -> sX[c][hy][hx]
template <int TY>
__device__ __forceinline__ void load_halo(const float *__restrict__ x, float *sX, const Tile &t, int Cin, int H, int W) {
    constexpr int HY = TY + 6;
    for (int i = threadIdx.x; i < Cin * HY * IC_HX; i += 256) {
        const int hx = i % IC_HX, r = i / IC_HX, hy = r % HY, c = r / HY;
        const int yy = t.y0 + hy - 3, xx = t.x0 + hx - 3;
        float v = 0.f;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) v = x[(((int64_t)t.b * Cin + c) * H + yy) * W + xx];
        sX[(c * HY + hy) * IC_LDX + hx] = v;
    }
}

// Forward.  grid (tile, block of 32 output channels); a tile is 8 x 32 pixels.  Thread (cog = tid & 7, px = tid >> 3) owns channels
// [4 cog, +4) of the block at column px of the tile, all 8 rows: 32 accumulators.  Per (plane, kw) the 14 halo values of its column
// are read once and serve the 7 x 8 (kh, row) pairs.  The order of an output's sum: bias, then (c, kw, kh) ascending.
constexpr int ICF_TY = 8, ICF_CB = 32;

__global__ __launch_bounds__(256) void init_fwd_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                      const float *__restrict__ bias, float *__restrict__ out, int Cin, int H, int W,
                                                      int Cout, int tiles_x, int tiles_y) {
    constexpr int HY = ICF_TY + 6;
    __shared__ __attribute__((aligned(16))) float sX[IC_MAXC * HY * IC_LDX];
    __shared__ __attribute__((aligned(16))) float sW[IC_MAXC * 49 * ICF_CB];        // [c][kh][kw][co of the block]
    const int tid = threadIdx.x, cog = tid & 7, px = tid >> 3;
    const int co0 = blockIdx.y * ICF_CB;
    const Tile t = tile_of(blockIdx.x, tiles_x, tiles_y, ICF_TY);
    load_halo<ICF_TY>(x, sX, t, Cin, H, W);
    for (int i = tid; i < Cin * 49 * ICF_CB; i += 256) {
        const int co = i % ICF_CB, k = i / ICF_CB;                        // k = (c 7 + kh) 7 + kw, as the weight's own order
        sW[i] = w[(int64_t)(co0 + co) * (Cin * 49) + k];
    }
    __syncthreads();
    f32x4 acc[ICF_TY];
    const f32x4 bv = *(const f32x4 *)(bias + co0 + 4 * cog);
#pragma unroll
    for (int r = 0; r < ICF_TY; ++r) acc[r] = bv;
    for (int c = 0; c < Cin; ++c) {
#pragma unroll
        for (int kw = 0; kw < 7; ++kw) {
            float col[HY];
#pragma unroll
            for (int hy = 0; hy < HY; ++hy) col[hy] = sX[(c * HY + hy) * IC_LDX + px + kw];
#pragma unroll
            for (int kh = 0; kh < 7; ++kh) {
                const f32x4 wv = *(const f32x4 *)(sW + ((c * 7 + kh) * 7 + kw) * ICF_CB + 4 * cog);
#pragma unroll
                for (int r = 0; r < ICF_TY; ++r) {
                    const float xv = col[r + kh];
                    acc[r].x = fmaf(wv.x, xv, acc[r].x);
                    acc[r].y = fmaf(wv.y, xv, acc[r].y);
                    acc[r].z = fmaf(wv.z, xv, acc[r].z);
                    acc[r].w = fmaf(wv.w, xv, acc[r].w);
                }
            }
        }
    }
    const int xx = t.x0 + px;
    if (xx >= W) return;
#pragma unroll
    for (int r = 0; r < ICF_TY; ++r) {
        const int yy = t.y0 + r;
        if (yy < H) *(f32x4 *)(out + (((int64_t)t.b * H + yy) * W + xx) * Cout + co0 + 4 * cog) = acc[r];
    }
}

// Weight gradient.  g[k][co], k = (c 7 + kh) 7 + kw for k < 49 Cin, and g[49 Cin][co] = dbias[co].
//   grid (split, block of CB output channels); split s owns the tiles [s tps, (s + 1) tps) and writes its partial [49 Cin + 1][Cout]
//   to the workspace, or to g itself when there is one split; two more launches add the partials in order (launch_sum).
//   A tile is TY x 32 pixels with TY CB = 256: its dout [pixel][CB] (32 KB) and its halo of x go to the LDS.
//   Thread (cog = tid % (CB / 4), slot = tid / (CB / 4)) owns channels [4 cog, +4) of the block and one row (c, kh) = slot of the
//   window, its 7 kw taps: 28 accumulators; slot 7 Cin sums dout itself (dbias); the slots beyond are idle (CB = 64: 16 slots for the
//   14 rows of 2 planes; CB = 32: 32 slots for the 21 rows of 3).  Per tile row the thread holds the 38 halo values of its window row
//   in registers; every pixel then costs one 16-byte LDS read of dout and 28 fmaf.
constexpr int IC_G = 32;                   // partials per launch_sum group

struct InitWgradPlan {
    int CB, TY, tiles_x, tiles_y, tps, S;
    int64_t ntiles, out;
};

InitWgradPlan init_wgrad_plan(int B, int Cin, int H, int W, int Cout) {
    InitWgradPlan p;
    p.CB = (Cin == 2 && Cout % 64 == 0) ? 64 : 32;
    p.TY = 256 / p.CB;
    p.tiles_x = (W + IC_TX - 1) / IC_TX;
    p.tiles_y = (H + p.TY - 1) / p.TY;
    p.ntiles = (int64_t)B * p.tiles_y * p.tiles_x;
    p.out = (int64_t)(49 * Cin + 1) * Cout;
    int64_t want = 1024 / (Cout / p.CB);                                  // four workgroups per CU: one loads while another computes
    if (want < 1) want = 1;
    if (want > p.ntiles) want = p.ntiles;
    p.tps = (int)((p.ntiles + want - 1) / want);
    p.S = (int)((p.ntiles + p.tps - 1) / p.tps);
    return p;
}

template <int CB>
__global__ __launch_bounds__(256) void init_wgrad_kernel(const float *__restrict__ x, const float *__restrict__ dout,
                                                        float *__restrict__ part, int Cin, int H, int W, int Cout, int tiles_x,
                                                        int tiles_y, int64_t ntiles, int tps) {
    constexpr int TY = 256 / CB, HY = TY + 6, NCOG = CB / 4, PIX = TY * IC_TX;
    constexpr int DV = PIX * NCOG / 256;                                  // 16-byte vectors of dout per thread and tile
    __shared__ __attribute__((aligned(16))) float sX[IC_MAXC * HY * IC_LDX];
    __shared__ __attribute__((aligned(16))) float sD[PIX * CB];
    const int tid = threadIdx.x, cog = tid % NCOG, slot = tid / NCOG;
    const int co0 = blockIdx.y * CB;
    const int rows = 7 * Cin;
    const bool tap_row = slot < rows, bias_row = slot == rows;
    const int c = tap_row ? slot / 7 : 0, kh = tap_row ? slot % 7 : 0;
    f32x4 acc[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int64_t t0 = (int64_t)blockIdx.x * tps, t1 = min(ntiles, t0 + tps);
    for (int64_t ti = t0; ti < t1; ++ti) {
        const Tile t = tile_of(ti, tiles_x, tiles_y, TY);
        __syncthreads();                                                  // the previous tile's reads are done
        load_halo<TY>(x, sX, t, Cin, H, W);
#pragma unroll
        for (int i = 0; i < DV; ++i) {
            const int idx = tid + 256 * i;
            const int v = idx % NCOG, p = idx / NCOG;
            const int yy = t.y0 + p / IC_TX, xx = t.x0 + p % IC_TX;
            f32x4 val = {0.f, 0.f, 0.f, 0.f};
            if (yy < H && xx < W) val = *(const f32x4 *)(dout + (((int64_t)t.b * H + yy) * W + xx) * Cout + co0 + 4 * v);
            *(f32x4 *)(sD + p * CB + 4 * v) = val;
        }
        __syncthreads();
        if (tap_row) {
#pragma unroll 1
            for (int r = 0; r < TY; ++r) {
                float row[IC_HX];
                const float *xr = sX + (c * HY + r + kh) * IC_LDX;
#pragma unroll
                for (int i = 0; i < IC_HX; ++i) row[i] = xr[i];
                const float *dr = sD + r * IC_TX * CB + 4 * cog;
#pragma unroll
                for (int px = 0; px < IC_TX; ++px) {
                    const f32x4 d = *(const f32x4 *)(dr + px * CB);
#pragma unroll
                    for (int kw = 0; kw < 7; ++kw) {
                        const float xv = row[px + kw];
                        acc[kw].x = fmaf(d.x, xv, acc[kw].x);
                        acc[kw].y = fmaf(d.y, xv, acc[kw].y);
                        acc[kw].z = fmaf(d.z, xv, acc[kw].z);
                        acc[kw].w = fmaf(d.w, xv, acc[kw].w);
                    }
                }
            }
        } else if (bias_row) {
            for (int p = 0; p < PIX; ++p) acc[0] += *(const f32x4 *)(sD + p * CB + 4 * cog);
        }
    }
    float *op = part + (int64_t)blockIdx.x * (49 * Cin + 1) * Cout + co0 + 4 * cog;
    if (tap_row) {
#pragma unroll
        for (int kw = 0; kw < 7; ++kw) *(f32x4 *)(op + (int64_t)((c * 7 + kh) * 7 + kw) * Cout) = acc[kw];
    } else if (bias_row) {
        *(f32x4 *)(op + (int64_t)(49 * Cin) * Cout) = acc[0];
    }
}

// ---- final_conv ----------------------------------------------------------------------------------------------------------------
// 16 lanes per pixel; lane l owns the 16-byte vectors l, l + 16, ... of the pixel's C channels, at most NV of them.
constexpr int FC_CHUNK = 1024;             // pixels per workgroup of the backward
constexpr int FC_G = 32;                   // partials per launch_sum group

// the sum of v over a pixel's 16 lanes, a fixed butterfly; every lane gets it
__device__ __forceinline__ float sum16(float v) {
#pragma unroll
    for (int m = 8; m > 0; m >>= 1) v += __shfl_xor(v, m, 16);
    return v;
}

// grid (groups of 16 pixels).  The order of a pixel's sum: per lane its vectors ascending, the four elements of a vector in order;
// then the butterfly; then the bias.
template <int NV>
__global__ __launch_bounds__(256) void final_fwd_kernel(const float *__restrict__ x, int ld, int off, const float *__restrict__ w,
                                                       const float *__restrict__ bias, float *__restrict__ out, int64_t npix, int C) {
    const int l = threadIdx.x & 15, nvec = C >> 2;
    const int64_t p = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    float s = 0.f;
    if (p < npix) {
        const float *xp = x + p * ld + off;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int v = l + 16 * j;
            if (v < nvec) {
                const f32x4 a = *(const f32x4 *)(xp + 4 * v), b = *(const f32x4 *)(w + 4 * v);
                s = fmaf(a.x, b.x, s);
                s = fmaf(a.y, b.y, s);
                s = fmaf(a.z, b.z, s);
                s = fmaf(a.w, b.w, s);
            }
        }
    }
    s = sum16(s);
    if (p < npix && l == 0) out[p] = s + bias[0];
}

// grid (chunk of FC_CHUNK pixels): dx = dout w (dense [npix][C]); part[chunk][q] = the chunk's sum of dout x[.][q] for q < C and of
// dout for q = C (row stride C + 4).  Pixel group gp = tid >> 4 takes the chunk's pixels gp, gp + 16, ... in order; the 16 groups are
// then added in order through the LDS.
template <int NV>
__global__ __launch_bounds__(256) void final_bwd_kernel(const float *__restrict__ x, int ld, int off, const float *__restrict__ w,
                                                       const float *__restrict__ dout, float *__restrict__ dx,
                                                       float *__restrict__ part, int64_t npix, int C) {
    __shared__ __attribute__((aligned(16))) float red[16 * 64];
    __shared__ float redb[16];
    const int tid = threadIdx.x, l = tid & 15, gp = tid >> 4, nvec = C >> 2;
    const int64_t p0 = (int64_t)blockIdx.x * FC_CHUNK, p1 = min(npix, p0 + FC_CHUNK);
    f32x4 wv[NV], acc[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int v = l + 16 * j;
        wv[j] = v < nvec ? *(const f32x4 *)(w + 4 * v) : f32x4{0.f, 0.f, 0.f, 0.f};
        acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float db = 0.f;
    for (int64_t p = p0 + gp; p < p1; p += 16) {
        const float d = dout[p];
        db += d;
        const float *xp = x + p * ld + off;
        float *dp = dx + p * C;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int v = l + 16 * j;
            if (v < nvec) {
                const f32x4 a = *(const f32x4 *)(xp + 4 * v);
                acc[j].x = fmaf(d, a.x, acc[j].x);
                acc[j].y = fmaf(d, a.y, acc[j].y);
                acc[j].z = fmaf(d, a.z, acc[j].z);
                acc[j].w = fmaf(d, a.w, acc[j].w);
                *(f32x4 *)(dp + 4 * v) = f32x4{d * wv[j].x, d * wv[j].y, d * wv[j].z, d * wv[j].w};
            }
        }
    }
    float *op = part + (int64_t)blockIdx.x * (C + 4);
    if (l == 0) redb[gp] = db;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        __syncthreads();                                                  // the previous round's reads are done
        *(f32x4 *)(red + gp * 64 + 4 * l) = acc[j];
        __syncthreads();
        const int q = 64 * j + tid;                                       // channel of this round, for tid < 64
        if (tid < 64 && q < C) {
            float s = 0.f;
#pragma unroll
            for (int g = 0; g < 16; ++g) s += red[g * 64 + tid];
            op[q] = s;
        }
    }
    if (tid == 0) {
        float s = 0.f;
        for (int g = 0; g < 16; ++g) s += redb[g];
        op[C] = s;
        op[C + 1] = op[C + 2] = op[C + 3] = 0.f;
    }
}

int fc_nv(int C) {
    const int need = (C / 4 + 15) / 16;
    int nv = 1;
    while (nv < need) nv *= 2;
    return nv;
}

// npix <= 2^30: the first-level sum of the backward has npix / (FC_CHUNK FC_G) rows on grid.y
bool fc_shape_ok(int64_t npix, int C) { return npix > 0 && npix <= (1ll << 30) && C > 0 && C % 4 == 0 && C <= 1024; }

bool ic_shape_ok(int B, int Cin, int H, int W, int Cout) {
    return B > 0 && B <= 65535 && (Cin == 2 || Cin == 3) && H > 0 && W > 0 && H <= 32768 && W <= 32768 && Cout > 0 && Cout % 32 == 0 &&
           Cout <= 512;
}

}  // namespace

extern "C" int fd_init_conv7_fwd_f32(const float *x, const float *weight, const float *bias, float *out, int B, int Cin, int H, int W,
                                     int Cout, void *stream) {
    FD_REQUIRE(x && weight && bias && out, "fd_init_conv7_fwd_f32: null pointer");
    FD_REQUIRE(ic_shape_ok(B, Cin, H, W, Cout),
               "fd_init_conv7_fwd_f32: unsupported shape B=%d Cin=%d H=%d W=%d Cout=%d (Cin 2 or 3, Cout a multiple of 32, at most 512)", B,
               Cin, H, W, Cout);
    FD_REQUIRE(al16(bias) && al16(out), "fd_init_conv7_fwd_f32: bias and out must be 16-byte aligned");
    const int tiles_x = (W + IC_TX - 1) / IC_TX, tiles_y = (H + ICF_TY - 1) / ICF_TY;
    const int64_t ntiles = (int64_t)B * tiles_y * tiles_x;
    FD_REQUIRE(ntiles < (1ll << 31), "fd_init_conv7_fwd_f32: unsupported shape (too many tiles: %lld)", (long long)ntiles);
    hipLaunchKernelGGL(init_fwd_kernel, dim3((unsigned)ntiles, (unsigned)(Cout / ICF_CB)), dim3(256), 0, (hipStream_t)stream, x, weight,
                       bias, out, Cin, H, W, Cout, tiles_x, tiles_y);
    FD_LAUNCH_OK("fd_init_conv7_fwd_f32");
    return FD_OK;
}

extern "C" int64_t fd_init_conv7_wgrad_ws_floats(int B, int Cin, int H, int W, int Cout) {
    if (!ic_shape_ok(B, Cin, H, W, Cout)) return 0;
    const InitWgradPlan p = init_wgrad_plan(B, Cin, H, W, Cout);
    return p.S > 1 ? (int64_t)(p.S + (p.S + IC_G - 1) / IC_G) * p.out : 4;
}

extern "C" int fd_init_conv7_wgrad_f32(const float *x, const float *dout, float *g, float *ws, int B, int Cin, int H, int W, int Cout,
                                       void *stream) {
    FD_REQUIRE(x && dout && g && ws, "fd_init_conv7_wgrad_f32: null pointer");
    FD_REQUIRE(ic_shape_ok(B, Cin, H, W, Cout),
               "fd_init_conv7_wgrad_f32: unsupported shape B=%d Cin=%d H=%d W=%d Cout=%d (Cin 2 or 3, Cout a multiple of 32, at most 512)",
               B, Cin, H, W, Cout);
    FD_REQUIRE(al16(dout) && al16(g) && al16(ws), "fd_init_conv7_wgrad_f32: dout, g and ws must be 16-byte aligned");
    const InitWgradPlan p = init_wgrad_plan(B, Cin, H, W, Cout);
    const hipStream_t st = (hipStream_t)stream;
    float *part = p.S > 1 ? ws : g;
    const dim3 grid((unsigned)p.S, (unsigned)(Cout / p.CB));
    if (p.CB == 64)
        hipLaunchKernelGGL(init_wgrad_kernel<64>, grid, dim3(256), 0, st, x, dout, part, Cin, H, W, Cout, p.tiles_x, p.tiles_y, p.ntiles,
                           p.tps);
    else
        hipLaunchKernelGGL(init_wgrad_kernel<32>, grid, dim3(256), 0, st, x, dout, part, Cin, H, W, Cout, p.tiles_x, p.tiles_y, p.ntiles,
                           p.tps);
    if (p.S > 1) {                                                        // the S partials in order, IC_G at a time, then the groups in order
        const int m1 = (p.S + IC_G - 1) / IC_G;
        float *stage = ws + (int64_t)p.S * p.out;
        launch_sum(ws, p.out, 0, p.S, (int)p.out, IC_G, stage, p.out, 0, 1, st);
        launch_sum(stage, p.out, 0, m1, (int)p.out, m1, g, p.out, 0, 1, st);
    }
    FD_LAUNCH_OK("fd_init_conv7_wgrad_f32");
    return FD_OK;
}

#define FD_FC_DISPATCH(KERNEL, ...)                                                                            \
    switch (fc_nv(C)) {                                                                                        \
    case 1: hipLaunchKernelGGL(KERNEL<1>, grid, dim3(256), 0, st, __VA_ARGS__); break;                         \
    case 2: hipLaunchKernelGGL(KERNEL<2>, grid, dim3(256), 0, st, __VA_ARGS__); break;                         \
    case 4: hipLaunchKernelGGL(KERNEL<4>, grid, dim3(256), 0, st, __VA_ARGS__); break;                         \
    case 8: hipLaunchKernelGGL(KERNEL<8>, grid, dim3(256), 0, st, __VA_ARGS__); break;                         \
    default: hipLaunchKernelGGL(KERNEL<16>, grid, dim3(256), 0, st, __VA_ARGS__); break;                       \
    }

static bool fc_layout_ok(const float *x, int ld, int off, int C) {
    return ld >= C && ld % 4 == 0 && off >= 0 && off % 4 == 0 && off + C <= ld && al16(x);
}

extern "C" int fd_final_conv1_fwd_f32(const float *x, int ld, int off, const float *weight, const float *bias, float *out, int64_t npix,
                                      int C, void *stream) {
    FD_REQUIRE(x && weight && bias && out, "fd_final_conv1_fwd_f32: null pointer");
    FD_REQUIRE(fc_shape_ok(npix, C), "fd_final_conv1_fwd_f32: unsupported shape npix=%lld C=%d (C a multiple of 4, at most 1024)",
               (long long)npix, C);
    FD_REQUIRE(fc_layout_ok(x, ld, off, C) && al16(weight), "fd_final_conv1_fwd_f32: unsupported layout ld=%d off=%d (multiples of 4, "
               "off + C <= ld, x and weight 16-byte aligned)", ld, off);
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((npix + 15) / 16));
    FD_FC_DISPATCH(final_fwd_kernel, x, ld, off, weight, bias, out, npix, C)
    FD_LAUNCH_OK("fd_final_conv1_fwd_f32");
    return FD_OK;
}

// workspace: the partials [nchunk][C + 4], then the first-level sums [ceil(nchunk / FC_G)][C + 4]
extern "C" int64_t fd_final_conv1_bwd_ws_floats(int64_t npix, int C) {
    if (!fc_shape_ok(npix, C)) return 0;
    const int64_t nchunk = (npix + FC_CHUNK - 1) / FC_CHUNK, m1 = (nchunk + FC_G - 1) / FC_G;
    return (nchunk + m1) * (C + 4);
}

// dwb [C + 4]: dweight, then dbias, then three zeros
extern "C" int fd_final_conv1_bwd_f32(const float *x, int ld, int off, const float *weight, const float *dout, float *dx, float *dwb,
                                      float *ws, int64_t npix, int C, void *stream) {
    FD_REQUIRE(x && weight && dout && dx && dwb && ws, "fd_final_conv1_bwd_f32: null pointer");
    FD_REQUIRE(fc_shape_ok(npix, C), "fd_final_conv1_bwd_f32: unsupported shape npix=%lld C=%d (C a multiple of 4, at most 1024)",
               (long long)npix, C);
    FD_REQUIRE(fc_layout_ok(x, ld, off, C) && al16(weight) && al16(dx), "fd_final_conv1_bwd_f32: unsupported layout ld=%d off=%d "
               "(multiples of 4, off + C <= ld, x, weight and dx 16-byte aligned)", ld, off);
    const hipStream_t st = (hipStream_t)stream;
    const int64_t nchunk = (npix + FC_CHUNK - 1) / FC_CHUNK, m1 = (nchunk + FC_G - 1) / FC_G;
    const int Q = C + 4;
    float *part = ws, *stage = ws + nchunk * Q;
    const dim3 grid((unsigned)nchunk);
    FD_FC_DISPATCH(final_bwd_kernel, x, ld, off, weight, dout, dx, part, npix, C)
    launch_sum(part, Q, 0, (int)nchunk, Q, FC_G, stage, Q, 0, 1, st);
    launch_sum(stage, Q, 0, (int)m1, Q, (int)m1, dwb, Q, 0, 1, st);
    FD_LAUNCH_OK("fd_final_conv1_bwd_f32");
    return FD_OK;
}
