// fd_resample_train.hip -- the two kernels that the backwards of the U-Net's resampling convolutions (src/DADiff.py:128-136:
// Downsample = Conv2d(4, 2, 1), Upsample = nearest x2 -> Conv2d(3, padding 1)) and the Upsample's forward had none for, for
// training, fp32, NHWC.  Write Down for the 4x4 / stride 2 / pad 1 convolution and Up for nearest x2 followed by 3x3 / pad 1: each
// is the other's transpose up to a fixed fold of the taps (founddiff_amd/resample_train.py holds the folds), so with
// fd_conv2d(FD_F32) for the Down-shaped products these two cover every pass of both:
//
//   fd_conv_sub2x_f32   out[b, 2i+a, 2j+b', n] = bias[n] + sum_{r,s,c} w2[n][2a+b'][r][s][c] in[b, i+a+r-1, j+b'+s-1, c]
//                       the Up forward (w2 = the 3x3 taps folded per parity class) and the Down input gradient (w2 = the 4x4 taps
//                       re-indexed: kh(0,0) = 3, kh(0,1) = 1, kh(1,0) = 2, kh(1,1) = 0)
//   fd_corr4x4s2_f32    g[p][t][u][q] = sum_{b,i,j} coarse[b,i,j,p] fine[b, 2i+t-1, 2j+u-1, q]
//                       the Down weight gradient as it is (coarse = dout, fine = x) and the Up weight gradient before its unfold
//                       (coarse = x, fine = dout)
//
// Exact fp32 on v_mfma_f32_16x16x4_f32 (an fmaf chain per output).  No float atomics; tile sizes, the split count and every order
// of summation depend on the shape only, and the sums of one slice do not depend on the batch in fd_conv_sub2x_f32.
//
// 1. fd_conv_sub2x_f32: four GEMMs (one per parity class) with M = Cout, N = source pixels, K = 4 Cin that share their B operand.
//      workgroup = 4 waves, a source tile of 8 x 16 pixels (16 x 32 output pixels) x 32 output channels; wave w owns output
//                  channels [16 (w & 1), +16) and source rows [4 (w >> 1), +4) of the tile: 4 classes x 4 rows = 16 accumulator
//                  tiles (64 VGPRs), an accumulator tile = 16 channels x the 16 pixels of one source row.
//      K step    = 32 input channels: the (8+2) x (16+2) halo of the source tile, [180 pixels][32 channels], in LDS with a row
//                  stride of 36 floats.  It serves all four classes and their 16 (class, tap) products; the next chunk's global
//                  loads are issued before the 2 x 256 MFMAs of the current one.  Inside a group of 16 channels the MFMA K index
//                  of lane group g, step j is channel 4 g + j, so a lane's B fragments of four K steps are one ds_read_b128
//                  (pixel stride 36 floats = 9 x 16 bytes: the 16 pixels of a row start in 16 different 4-bank groups; the two
//                  lane groups g that share a ds_read_b128 service group overlap 2-way in at most two of them -- 18 such reads
//                  per 256 MFMAs) and its A fragments one 16-byte global load of w2 (a row of 16 lanes reads 64 contiguous bytes;
//                  w2 is small and stays in L2: 64 MACs per weight byte read).
//      Traffic   : in x (Cout / 32) (+ 41 % halo) + out once + w2 once per pixel tile, from L2.
// 2. fd_corr4x4s2_f32: a GEMM with M = P, N = 16 Q, K = B H W coarse pixels: the tap correlation of fd_train_common.h, as
//    fd_conv3x3_wgrad_f32, here tapcorr_kernel<KT = 4 taps per axis, STRIDE = 2, TY x TX = 4 x 8 coarse pixels per K step, LDB = 40
//    floats per halo row in LDS> with f = fine read densely (ld = Q, off = 0).
//      workgroup = 4 waves, output tile 64 p x 16 taps x 32 q; wave w owns p in [16 w, +16): 32 accumulator tiles (128 AGPRs).
//      K step    = coarse [32][64] and the (2*4+2) x (2*8+2) halo of fine [180][32] in LDS (the four coarse pixels of one MFMA K
//                  step are two fine pixels apart, 80 floats, and fall into different banks); the halo serves all 16 taps.  The
//                  next tile's global loads are issued before the 8 x 32 MFMAs of the current one.
//      split K   : S = min(tiles, ceil(1024 / output tiles), 256, (coarse + fine elements) / (2 x 16 P Q)) contiguous ranges of
//                  the pixel tiles: the partials never take more than half of what the two activations do (256 splits at down0, 3
//                  of 8 MB each at ups0); tapcorr_reduce_kernel adds them in order.  S = 1 (one pixel tile) writes g directly.
//      Traffic   : coarse x (Q / 32) + fine x ceil(P / 64) (+ 41 % halo) + 2 S partials.
#include "fd_train_common.h"

namespace {

bool chan_ok(int c) { return c > 0 && c % 32 == 0 && c <= 512; }

// ---- 1. sub-pixel convolution --------------------------------------------------------------------------------------------------
constexpr int SX_TY = 8, SX_TX = 16, SX_HX = SX_TX + 2, SX_HY = SX_TY + 2, SX_HPIX = SX_HX * SX_HY;
constexpr int SX_NB = 32, SX_CB = 32, SX_LD = 36;
constexpr int SX_BV = (SX_HPIX * (SX_CB / 4) + 255) / 256;               // 16-byte vectors of the halo per thread and chunk: 6

bool sx_shape_ok(int B, int H, int W, int Cin, int Cout) {
    return B > 0 && H > 0 && W > 0 && H < (1 << 29) && W < (1 << 29) && chan_ok(Cin) && chan_ok(Cout) &&
           (int64_t)B * ((H + SX_TY - 1) / SX_TY) * ((W + SX_TX - 1) / SX_TX) < (1ll << 31);
}

// grid (pixel tile of (b, ty, tx), block of 32 output channels)
__global__ __launch_bounds__(256) void sub2x_kernel(const float *__restrict__ in, const float *__restrict__ w2,
                                                   const float *__restrict__ bias, float *__restrict__ out, int H, int W, int Cin,
                                                   int Cout, int tiles_x, int tiles_y) {
    __shared__ __attribute__((aligned(16))) float sB[SX_HPIX * SX_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, r = lane & 15;
    const int n0 = blockIdx.y * SX_NB + 16 * (wave & 1), row0 = 4 * (wave >> 1);
    const int tx = (int)(blockIdx.x % tiles_x);
    const int64_t tq = blockIdx.x / tiles_x;
    const int ty = (int)(tq % tiles_y);
    const int64_t b = tq / tiles_y;
    const int y0 = ty * SX_TY, x0 = tx * SX_TX;
    f32x4 acc[4][4];                                                     // [class][source row]
    {
        f32x4 bv = {0.f, 0.f, 0.f, 0.f};
        if (bias) bv = *(const f32x4 *)(bias + n0 + 4 * g);
#pragma unroll
        for (int cls = 0; cls < 4; ++cls)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[cls][i] = bv;
    }
    f32x4 rb[SX_BV];
    auto gload = [&](int c_base) {
#pragma unroll
        for (int i = 0; i < SX_BV; ++i) {
            const int idx = tid + 256 * i;
            const int v = idx & 7, p = idx >> 3;
            const int hy = p / SX_HX, hx = p - hy * SX_HX;
            const int yy = y0 + hy - 1, xx = x0 + hx - 1;
            f32x4 val = {0.f, 0.f, 0.f, 0.f};
            if (p < SX_HPIX && yy >= 0 && yy < H && xx >= 0 && xx < W)
                val = *(const f32x4 *)(in + ((b * H + yy) * W + xx) * Cin + c_base + 4 * v);
            rb[i] = val;
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int i = 0; i < SX_BV; ++i) {
            const int idx = tid + 256 * i;
            if ((idx >> 3) < SX_HPIX) *(f32x4 *)(sB + (idx >> 3) * SX_LD + 4 * (idx & 7)) = rb[i];
        }
    };
    // lane (g, r): A[n = n0 + r][k], B[k][pixel = r of a source row], k = channel 4 g + j of the group of 16 in MFMA step j
    const float *wp = w2 + (int64_t)(n0 + r) * 16 * Cin + 4 * g;
    const float *bp = sB + (row0 * SX_HX + r) * SX_LD + 4 * g;
    gload(0);
    for (int c_base = 0; c_base < Cin; c_base += SX_CB) {
        __syncthreads();                       // the previous chunk's fragment reads are done
        lstore();
        __syncthreads();
        if (c_base + SX_CB < Cin) gload(c_base + SX_CB);
#pragma unroll
        for (int kg = 0; kg < SX_CB; kg += 16) {
            f32x4 bv[6][3];
#pragma unroll
            for (int hr = 0; hr < 6; ++hr)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) bv[hr][dx] = *(const f32x4 *)(bp + (hr * SX_HX + dx) * SX_LD + kg);
#pragma unroll
            for (int cls = 0; cls < 4; ++cls)
#pragma unroll
                for (int tap = 0; tap < 4; ++tap) {
                    const f32x4 aw = *(const f32x4 *)(wp + (cls * 4 + tap) * Cin + c_base + kg);
                    const int dy = (cls >> 1) + (tap >> 1), dx = (cls & 1) + (tap & 1);
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            acc[cls][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(aw[j], bv[i + dy][dx][j], acc[cls][i], 0, 0, 0);
                }
        }
    }
    // D: lane (g, r) holds channels n0 + 4 g + (0..3) of pixel r
    const int xx = x0 + r;
    if (xx >= W) return;
    const int64_t OW = 2 * (int64_t)W;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int yy = y0 + row0 + i;
        if (yy >= H) continue;
#pragma unroll
        for (int cls = 0; cls < 4; ++cls) {
            const int64_t oy = 2 * (int64_t)yy + (cls >> 1), ox = 2 * (int64_t)xx + (cls & 1);
            *(f32x4 *)(out + ((b * 2 * H + oy) * OW + ox) * Cout + n0 + 4 * g) = acc[cls][i];
        }
    }
}

// ---- 2. the 4x4 / stride 2 correlation -----------------------------------------------------------------------------------------
constexpr int CR_TY = 4, CR_TX = 8;
constexpr auto cr_launch = tapcorr_launch<4, 2, CR_TY, CR_TX, 40>;

bool cr_shape_ok(int B, int H, int W, int P, int Q) {
    return B > 0 && H > 0 && W > 0 && H < (1 << 29) && W < (1 << 29) && chan_ok(P) && chan_ok(Q) &&
           (int64_t)B * ((H + CR_TY - 1) / CR_TY) * ((W + CR_TX - 1) / CR_TX) < (1ll << 31);
}

TapPlan cr_plan(int B, int H, int W, int P, int Q) {
    // partials <= half the two activations
    const int64_t cap = (int64_t)B * H * W * (P + 4 * (int64_t)Q) / (2 * (int64_t)P * 16 * Q);
    return tap_plan(4, CR_TY, CR_TX, B, H, W, P, Q, cap);
}

}  // namespace

extern "C" int fd_conv_sub2x_f32(const float *in, const float *w2, const float *bias, float *out, int B, int H, int W, int Cin,
                                 int Cout, void *stream) {
    FD_REQUIRE(in && w2 && out, "fd_conv_sub2x_f32: null pointer");
    FD_REQUIRE(sx_shape_ok(B, H, W, Cin, Cout),
               "fd_conv_sub2x_f32: unsupported shape B=%d H=%d W=%d Cin=%d Cout=%d (Cin, Cout %% 32 == 0, at most 512)", B, H, W, Cin,
               Cout);
    FD_REQUIRE(al16(in) && al16(w2) && al16(bias) && al16(out), "fd_conv_sub2x_f32: tensors must be 16-byte aligned");
    const int tiles_x = (W + SX_TX - 1) / SX_TX, tiles_y = (H + SX_TY - 1) / SX_TY;
    hipLaunchKernelGGL(sub2x_kernel, dim3((unsigned)((int64_t)B * tiles_y * tiles_x), (unsigned)(Cout / SX_NB)), dim3(256), 0,
                       (hipStream_t)stream, in, w2, bias, out, H, W, Cin, Cout, tiles_x, tiles_y);
    FD_LAUNCH_OK("fd_conv_sub2x_f32");
    return FD_OK;
}

extern "C" int64_t fd_corr4x4s2_ws_floats(int B, int H, int W, int P, int Q) {
    if (!cr_shape_ok(B, H, W, P, Q)) return 0;
    return tap_ws_floats(cr_plan(B, H, W, P, Q));
}

extern "C" int fd_corr4x4s2_f32(const float *coarse, const float *fine, float *g, float *ws, int B, int H, int W, int P, int Q,
                                void *stream) {
    FD_REQUIRE(coarse && fine && g && ws, "fd_corr4x4s2_f32: null pointer");
    FD_REQUIRE(cr_shape_ok(B, H, W, P, Q),
               "fd_corr4x4s2_f32: unsupported shape B=%d H=%d W=%d P=%d Q=%d (P, Q %% 32 == 0, at most 512)", B, H, W, P, Q);
    FD_REQUIRE(al16(coarse) && al16(fine) && al16(g) && al16(ws), "fd_corr4x4s2_f32: tensors must be 16-byte aligned");
    cr_launch(cr_plan(B, H, W, P, Q), coarse, fine, Q, 0, g, ws, H, W, P, Q, (hipStream_t)stream);
    FD_LAUNCH_OK("fd_corr4x4s2_f32");
    return FD_OK;
}
