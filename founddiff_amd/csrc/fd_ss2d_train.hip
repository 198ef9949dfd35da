// fd_ss2d_train.hip -- what the reference's SS2D.forward (src/emamba2.py:713-751) does around cross_selective_scan, for training,
// fp32, NHWC, on the halves of in_proj's output xz [B,H,W,2D] in place:
//
//   fd_dwconv3x3_silu_bwd_f32   backward of xc = SiLU(dwconv3x3(x) + bias)     (the forward is fd_dwconv3x3 with silu = 1)
//   fd_dwconv3x3_bwd_f32        the same without the activation (TransposedAttention's qkv_dwconv): dout is only read
//   fd_ln_silu_gate_fwd_f32     out = LN(y) * SiLU(z) + local[b]               (out_norm, the gate, + local; 2 floats of
//   fd_ln_silu_gate_bwd_f32     its backward                                     LayerNorm statistics kept per pixel)
//
// All three are streaming kernels: lane = 4 consecutive channels, 16-byte loads and stores along the channel axis.  Parameter
// gradients are per-workgroup partials in the workspace, summed by dwb/lsg-independent launches of partial_sum_kernel
// (fd_train_common.h) in a fixed order (no float atomics): bit-repeatable.  Tile sizes, rows per workgroup and every order of
// summation that concerns one slice depend on (H, W, C) only, never on the batch.
//
// 1. dwconv + SiLU backward, two launches over the activation:
//      pre:  workgroup = tpb tiles of 8 x 16 pixels x 64 channels; the (8+2) x (16+2) halo of x in LDS (x is read 1.41 times),
//            pre = conv(x) + bias recomputed (a 3 x 3 register window slides down the column), dpre = dout SiLU'(pre) written
//            OVER dout, the tile's dweight[t] += dpre x[p + t] and dbias += dpre in registers, summed over the 16 columns
//            through LDS in column order -> one partial row [10][64] per workgroup
//      dx:   dx = dwconv3x3(dpre) with the taps mirrored (fd_dwconv3x3's fp32 kernel: dpre read 1.41 times), written with dx's
//            own pixel stride / channel offset (the x half of dxz)
//    Traffic at down0, batch 2 (activation A = 268 MB): algorithmic 3 A (x, dout in, dx out); this form 1.41 A + A + A in the
//    first launch, 1.41 A + A in the second = 5.8 A.  (One launch needs dpre on a one-pixel halo, i.e. x on a two-pixel halo
//    and dout on a one-pixel halo: (12 x 20 + 10 x 18) / 128 + 1 = 4.3 A at this tile, in 76 KB of LDS per 64 channels.)
// 2. LN + SiLU gate, one launch each way (+ the partial sums): a row (pixel) sits in lpr = 16 / 32 / 64 neighbouring lanes,
//    VPL 16-byte vectors per lane; two-pass statistics in registers.  Forward: y, z in, out out = 3 A (algorithmic).  Backward:
//    dout, y, z in, dy, dz out = 5 A (algorithmic); dgamma / dbeta / dlocal ride in registers over the rows of a workgroup.
#include "fd_train_common.h"

namespace {

// ---- 1. SiLU(dwconv3x3 + bias) backward ----------------------------------------------------------------------------------
constexpr int DB_TY = 8, DB_TX = 16, DB_CB = 64, DB_HX = DB_TX + 2, DB_HY = DB_TY + 2, DB_G = 32;

struct DwbPlan {
    int tiles_x, tiles_y, cblocks, tpb, ngx;
    int64_t M, M1, part, stage, wflip, total;     // partial rows, after the first sum; floats of each workspace piece
};

DwbPlan dwb_plan(int B, int H, int W, int C) {
    DwbPlan p;
    p.tiles_x = (W + DB_TX - 1) / DB_TX;
    p.tiles_y = (H + DB_TY - 1) / DB_TY;
    p.cblocks = C / DB_CB;
    // tiles per workgroup (along x): fewer partial rows while one slice still gives the chip >= 1024 workgroups
    p.tpb = 1;
    while (p.tpb < 8 && 2 * p.tpb <= p.tiles_x && (int64_t)p.tiles_x * p.tiles_y * p.cblocks / (2 * p.tpb) >= 1024) p.tpb *= 2;
    p.ngx = (p.tiles_x + p.tpb - 1) / p.tpb;
    p.M = (int64_t)B * p.tiles_y * p.ngx;
    p.M1 = (p.M + DB_G - 1) / DB_G;
    p.part = round4(p.M * 10 * C);
    p.stage = round4(p.M1 * 10 * C);
    p.wflip = round4((int64_t)9 * C);
    p.total = p.part + p.stage + p.wflip;
    return p;
}

bool dwb_shape_ok(int B, int H, int W, int C) {
    return B > 0 && H > 0 && W > 0 && C > 0 && C % 64 == 0 && (int64_t)H * W < (1ll << 31) &&
           (int64_t)B * ((H + DB_TY - 1) / DB_TY) * ((W + DB_TX - 1) / DB_TX) < (1ll << 31) && B < 65536 &&
           (H + DB_TY - 1) / DB_TY < 65536;
}

// SILU = false: the linear conv (qkv_dwconv): dpre = dout, which is only read
template <bool SILU>
__global__ __launch_bounds__(256) void dwb_pre_kernel(const float *__restrict__ x, int ld_in, int off_in,
                                                     const float *__restrict__ w, const float *__restrict__ bias,
                                                     float *__restrict__ dout, float *__restrict__ part, int H, int W, int C,
                                                     int cblocks, int tpb, int ngx, int tiles_x) {
    __shared__ __attribute__((aligned(16))) float tile[DB_HY * DB_HX * DB_CB];      // also the [16][10][64] column partials
    const int tid = threadIdx.x;
    const int cb = blockIdx.x % cblocks, gx = blockIdx.x / cblocks;
    const int64_t img = blockIdx.z;
    const int y0 = blockIdx.y * DB_TY;
    const int cq = tid & 15, px = tid >> 4;
    const int c0 = cb * DB_CB + 4 * cq;
    f32x4 wt[9], dw[9], bs = {0.f, 0.f, 0.f, 0.f}, db = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        wt[t] = *(const f32x4 *)(w + (int64_t)t * C + c0);
        dw[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (bias) bs = *(const f32x4 *)(bias + c0);
    for (int it = 0; it < tpb; ++it) {
        const int tx = gx * tpb + it;
        if (tx >= tiles_x) break;
        const int x0 = tx * DB_TX;
        __syncthreads();
        for (int idx = tid; idx < DB_HY * DB_HX * (DB_CB / 4); idx += 256) {
            const int v = idx & 15, pxl = idx >> 4;
            const int hy = pxl / DB_HX, hx = pxl - hy * DB_HX;
            const int yy = y0 + hy - 1, xx = x0 + hx - 1;
            f32x4 val = {0.f, 0.f, 0.f, 0.f};
            if (yy >= 0 && yy < H && xx >= 0 && xx < W)
                val = *(const f32x4 *)(x + ((img * H + yy) * W + xx) * ld_in + off_in + cb * DB_CB + 4 * v);
            *(f32x4 *)(tile + pxl * DB_CB + 4 * v) = val;
        }
        __syncthreads();
        const int xo = x0 + px;
        f32x4 rw[3][3];
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) rw[dy][dx] = *(const f32x4 *)(tile + (dy * DB_HX + px + dx) * DB_CB + 4 * cq);
#pragma unroll
        for (int r = 0; r < DB_TY; ++r) {
#pragma unroll
            for (int dx = 0; dx < 3; ++dx)
                rw[(r + 2) % 3][dx] = *(const f32x4 *)(tile + ((r + 2) * DB_HX + px + dx) * DB_CB + 4 * cq);
            f32x4 pre = bs;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) pre += rw[(r + dy) % 3][dx] * wt[dy * 3 + dx];
            const int yo = y0 + r;
            const bool ok = xo < W && yo < H;
            f32x4 d = {0.f, 0.f, 0.f, 0.f};
            if (ok) {
                float *gp = dout + ((img * H + yo) * W + xo) * C + c0;
                const f32x4 g = *(const f32x4 *)gp;
                if constexpr (SILU) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float s = sigmoid_f(pre[e]);
                        d[e] = g[e] * (s * (1.0f + pre[e] * (1.0f - s)));
                    }
                    *(f32x4 *)gp = d;
                } else {
                    d = g;
                }
            }
            db += d;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) dw[dy * 3 + dx] += d * rw[(r + dy) % 3][dx];
        }
    }
    // the 16 columns' sums, in column order
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 9; ++t) *(f32x4 *)(tile + (px * 10 + t) * DB_CB + 4 * cq) = dw[t];
    *(f32x4 *)(tile + (px * 10 + 9) * DB_CB + 4 * cq) = db;
    __syncthreads();
    if (tid < 10 * 16) {
        const int t = tid >> 4, q = tid & 15;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        for (int p = 0; p < 16; ++p) v += *(const f32x4 *)(tile + (p * 10 + t) * DB_CB + 4 * q);
        const int64_t m = (img * gridDim.y + blockIdx.y) * ngx + gx;
        *(f32x4 *)(part + (m * 10 + t) * C + cb * DB_CB + 4 * q) = v;
    }
}

__global__ __launch_bounds__(256) void dwb_flip_kernel(const float *__restrict__ w, float *__restrict__ wf, int C) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 9 * C) return;
    const int t = i / C, c = i - t * C;
    wf[i] = w[(8 - t) * C + c];
}

// ---- 2. out = LN(y) * SiLU(z) + local[b] ---------------------------------------------------------------------------------
struct LsgPlan {
    int lpr, vpl, rpb, ch, nchunk, M1;
    int64_t part, stage, fin, total;
};

constexpr int LSG_G = 16;

bool lsg_shape_ok(int B, int64_t hw, int C) { return B > 0 && B < 65536 && hw > 0 && hw < (1ll << 31) && C > 0 && C % 64 == 0 && C <= 1024; }

LsgPlan lsg_plan(int B, int64_t hw, int C) {
    LsgPlan p;
    p.lpr = C / 4 <= 16 ? 16 : (C / 4 <= 32 ? 32 : 64);
    p.vpl = (C + 4 * p.lpr - 1) / (4 * p.lpr);
    if (p.vpl == 3) p.vpl = 4;
    p.rpb = 256 / p.lpr;
    // rows per workgroup of the backward: ~512 workgroups from one slice, 16 .. 512 rows each (a function of hw alone)
    int64_t ch = ((hw + 511) / 512 + 15) / 16 * 16;
    p.ch = (int)(ch < 16 ? 16 : (ch > 512 ? 512 : ch));
    p.nchunk = (int)((hw + p.ch - 1) / p.ch);
    p.M1 = (p.nchunk + LSG_G - 1) / LSG_G;
    p.part = round4((int64_t)B * p.nchunk * 3 * C);
    p.stage = round4((int64_t)B * p.M1 * 3 * C);
    p.fin = round4((int64_t)B * 3 * C);
    p.total = p.part + p.stage + p.fin;
    return p;
}

__device__ __forceinline__ float group_sum(float t, int lpr) {
    for (int o = 1; o < lpr; o <<= 1) t += __shfl_xor(t, o, 64);
    return t;
}

template <int VPL>
__global__ __launch_bounds__(256) void lsg_fwd_kernel(const float *__restrict__ y, const float *__restrict__ gamma,
                                                     const float *__restrict__ beta, float eps, const float *__restrict__ z,
                                                     int ldz, int offz, const float *__restrict__ local, int local_ld,
                                                     float *__restrict__ out, float *__restrict__ stats, int64_t hw, int C, int lpr,
                                                     int64_t nrows) {
    const int tid = threadIdx.x, sub = tid % lpr;
    const int64_t row = (int64_t)blockIdx.x * (256 / lpr) + tid / lpr;
    const bool active = row < nrows;
    const int64_t rr = active ? row : 0;
    const int64_t b = rr / hw;
    const float invC = 1.0f / (float)C;
    f32x4 v[VPL];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int c = (j * lpr + sub) * 4;
        v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < C) v[j] = *(const f32x4 *)(y + rr * C + c);
        s += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
    }
    const float mean = group_sum(s, lpr) * invC;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int c = (j * lpr + sub) * 4;
        if (c < C) {
            v[j] -= mean;
            q += (v[j][0] * v[j][0] + v[j][1] * v[j][1]) + (v[j][2] * v[j][2] + v[j][3] * v[j][3]);
        }
    }
    const float rstd = rsqrtf(group_sum(q, lpr) * invC + eps);
    if (!active) return;
    if (sub == 0) {
        stats[2 * row] = mean;
        stats[2 * row + 1] = rstd;
    }
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int c = (j * lpr + sub) * 4;
        if (c >= C) continue;
        const f32x4 g = *(const f32x4 *)(gamma + c), bt = *(const f32x4 *)(beta + c);
        const f32x4 zz = *(const f32x4 *)(z + rr * ldz + offz + c);
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        if (local) o = *(const f32x4 *)(local + b * local_ld + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] += (v[j][e] * rstd * g[e] + bt[e]) * (zz[e] * sigmoid_f(zz[e]));
        *(f32x4 *)(out + rr * C + c) = o;
    }
}

// grid (chunk, b): rows [chunk ch, +ch) of slice b, rpb rows at a time; part[b][chunk][dgamma C | dbeta C | dlocal C]
template <int VPL>
__global__ __launch_bounds__(256) void lsg_bwd_kernel(const float *__restrict__ dout, const float *__restrict__ y,
                                                     const float *__restrict__ stats, const float *__restrict__ gamma,
                                                     const float *__restrict__ beta, const float *__restrict__ z, int ldz, int offz,
                                                     float *__restrict__ dy, float *__restrict__ dz, int lddz, int offdz,
                                                     float *__restrict__ part, int64_t hw, int C, int lpr, int ch) {
    __shared__ __attribute__((aligned(16))) float red[3 * 1024 * VPL];      // [row slot][3][lpr 4 VPL]
    const int tid = threadIdx.x, sub = tid % lpr, slot = tid / lpr, rpb = 256 / lpr;
    const int64_t b = blockIdx.y;
    const int64_t r0 = (int64_t)blockIdx.x * ch;
    const float invC = 1.0f / (float)C;
    f32x4 gm[VPL], bt[VPL], ag[VPL], ab[VPL], al[VPL];
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int c = (j * lpr + sub) * 4;
        gm[j] = bt[j] = ag[j] = ab[j] = al[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < C) {
            gm[j] = *(const f32x4 *)(gamma + c);
            bt[j] = *(const f32x4 *)(beta + c);
        }
    }
    for (int rr = slot; rr < ch; rr += rpb) {
        const bool active = r0 + rr < hw;
        const int64_t row = b * hw + (active ? r0 + rr : 0);
        const float mean = stats[2 * row], rstd = stats[2 * row + 1];
        f32x4 n[VPL], dn[VPL];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const int c = (j * lpr + sub) * 4;
            n[j] = dn[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (c < C && active) {
                const f32x4 yv = *(const f32x4 *)(y + row * C + c);
                const f32x4 g = *(const f32x4 *)(dout + row * C + c);
                const f32x4 zz = *(const f32x4 *)(z + row * ldz + offz + c);
                f32x4 dzv;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float nn = (yv[e] - mean) * rstd;
                    const float ln = nn * gm[j][e] + bt[j][e];
                    const float sg = sigmoid_f(zz[e]);
                    const float dln = g[e] * (zz[e] * sg);
                    dzv[e] = g[e] * ln * (sg * (1.0f + zz[e] * (1.0f - sg)));
                    n[j][e] = nn;
                    dn[j][e] = dln * gm[j][e];
                    ag[j][e] += dln * nn;
                    ab[j][e] += dln;
                    al[j][e] += g[e];
                }
                *(f32x4 *)(dz + row * lddz + offdz + c) = dzv;
                s1 += (dn[j][0] + dn[j][1]) + (dn[j][2] + dn[j][3]);
                s2 += (dn[j][0] * n[j][0] + dn[j][1] * n[j][1]) + (dn[j][2] * n[j][2] + dn[j][3] * n[j][3]);
            }
        }
        s1 = group_sum(s1, lpr) * invC;
        s2 = group_sum(s2, lpr) * invC;
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const int c = (j * lpr + sub) * 4;
            if (c < C && active) {
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = rstd * (dn[j][e] - s1 - n[j][e] * s2);
                *(f32x4 *)(dy + row * C + c) = o;
            }
        }
    }
    // the row slots' column sums, in slot order
    const int cw = lpr * 4 * VPL;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int c = (j * lpr + sub) * 4;
        *(f32x4 *)(red + (slot * 3 + 0) * cw + c) = ag[j];
        *(f32x4 *)(red + (slot * 3 + 1) * cw + c) = ab[j];
        *(f32x4 *)(red + (slot * 3 + 2) * cw + c) = al[j];
    }
    __syncthreads();
    float *pp = part + (b * gridDim.x + blockIdx.x) * 3 * C;
    for (int idx = tid; idx < 3 * C; idx += 256) {
        const int which = idx / C, c = idx - which * C;
        float v = 0.f;
        for (int sl = 0; sl < rpb; ++sl) v += red[(sl * 3 + which) * cw + c];
        pp[idx] = v;
    }
}

// fin [B][dgamma | dbeta | dlocal] -> dgamma, dbeta (sums over b in order), dlocal [B][C]
__global__ __launch_bounds__(256) void lsg_finish_kernel(const float *__restrict__ fin, int B, int C, float *__restrict__ dgamma,
                                                        float *__restrict__ dbeta, float *__restrict__ dlocal) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float g = 0.f, bt = 0.f;
    for (int b = 0; b < B; ++b) {
        g += fin[(int64_t)b * 3 * C + c];
        bt += fin[(int64_t)b * 3 * C + C + c];
        if (dlocal) dlocal[(int64_t)b * C + c] = fin[(int64_t)b * 3 * C + 2 * C + c];
    }
    dgamma[c] = g;
    dbeta[c] = bt;
}

}  // namespace

extern "C" int64_t fd_dwconv3x3_silu_bwd_ws_floats(int B, int H, int W, int C) {
    if (!dwb_shape_ok(B, H, W, C)) return 0;
    return dwb_plan(B, H, W, C).total;
}

// the two backwards of fd_dwconv3x3's fp32 form: name = the entry point, for its messages
template <bool SILU>
static int dwb_run(const char *name, const float *x, int ld_in, int off_in, const float *weight, const float *bias, float *dout,
                   float *dx, int ld_dx, int off_dx, float *dweight, float *dbias, float *ws, int B, int H, int W, int C,
                   void *stream) {
    FD_REQUIRE(x && weight && dout && dx && dweight && ws, "%s: null pointer", name);
    FD_REQUIRE((bias == nullptr) == (dbias == nullptr), "%s: dbias must be NULL exactly when bias is", name);
    FD_REQUIRE(dwb_shape_ok(B, H, W, C), "%s: unsupported shape B=%d H=%d W=%d C=%d (C %% 64 == 0)", name, B, H, W, C);
    FD_REQUIRE(ld_in >= off_in + C && ld_dx >= off_dx + C && off_in >= 0 && off_dx >= 0 && ld_in % 8 == 0 && off_in % 8 == 0 &&
                   ld_dx % 8 == 0 && off_dx % 8 == 0,
               "%s: strides / offsets must be multiples of 8 with off + C <= ld (ld_in=%d off_in=%d ld_dx=%d off_dx=%d)", name, ld_in,
               off_in, ld_dx, off_dx);
    FD_REQUIRE(al16(x) && al16(weight) && al16(bias) && al16(dout) && al16(dx) && al16(ws), "%s: tensors must be 16-byte aligned", name);
    const hipStream_t st = (hipStream_t)stream;
    const DwbPlan p = dwb_plan(B, H, W, C);
    float *part = ws, *stage = part + p.part, *wflip = stage + p.stage;
    hipLaunchKernelGGL(dwb_flip_kernel, dim3((unsigned)((9 * C + 255) / 256)), dim3(256), 0, st, weight, wflip, C);
    hipLaunchKernelGGL(dwb_pre_kernel<SILU>, dim3((unsigned)(p.ngx * p.cblocks), (unsigned)p.tiles_y, (unsigned)B), dim3(256), 0, st, x,
                       ld_in, off_in, weight, bias, dout, part, H, W, C, p.cblocks, p.tpb, p.ngx, p.tiles_x);
    launch_sum(part, 10 * (int64_t)C, 0, (int)p.M, 10 * C, DB_G, stage, 10 * (int64_t)C, 0, 1, st);
    launch_sum(stage, 10 * (int64_t)C, 0, (int)p.M1, 9 * C, (int)p.M1, dweight, 0, 0, 1, st);
    if (dbias) launch_sum(stage + 9 * (int64_t)C, 10 * (int64_t)C, 0, (int)p.M1, C, (int)p.M1, dbias, 0, 0, 1, st);
    FD_LAUNCH_OK(name);
    // dx = the mirrored taps over dpre
    return fd_dwconv3x3(FD_F32, dout, C, 0, wflip, nullptr, 0, dx, ld_dx, off_dx, B, H, W, C, stream);
}

extern "C" int fd_dwconv3x3_silu_bwd_f32(const float *x, int ld_in, int off_in, const float *weight, const float *bias, float *dout,
                                         float *dx, int ld_dx, int off_dx, float *dweight, float *dbias, float *ws, int B, int H,
                                         int W, int C, void *stream) {
    return dwb_run<true>("fd_dwconv3x3_silu_bwd_f32", x, ld_in, off_in, weight, bias, dout, dx, ld_dx, off_dx, dweight, dbias, ws, B,
                         H, W, C, stream);
}

extern "C" int64_t fd_dwconv3x3_bwd_ws_floats(int B, int H, int W, int C) { return fd_dwconv3x3_silu_bwd_ws_floats(B, H, W, C); }

// (the kernel takes dout through the pointer type of the SiLU form and, with SILU = false, only reads it)
extern "C" int fd_dwconv3x3_bwd_f32(const float *x, int ld_in, int off_in, const float *weight, const float *bias, const float *dout,
                                    float *dx, int ld_dx, int off_dx, float *dweight, float *dbias, float *ws, int B, int H, int W,
                                    int C, void *stream) {
    return dwb_run<false>("fd_dwconv3x3_bwd_f32", x, ld_in, off_in, weight, bias, const_cast<float *>(dout), dx, ld_dx, off_dx, dweight,
                          dbias, ws, B, H, W, C, stream);
}

#define FD_LSG_VPL(KERNEL, ...)                                                                      \
    do {                                                                                             \
        if (p.vpl == 1) hipLaunchKernelGGL(KERNEL<1>, __VA_ARGS__);                                  \
        else if (p.vpl == 2) hipLaunchKernelGGL(KERNEL<2>, __VA_ARGS__);                             \
        else hipLaunchKernelGGL(KERNEL<4>, __VA_ARGS__);                                             \
    } while (0)

extern "C" int fd_ln_silu_gate_fwd_f32(const float *y, const float *gamma, const float *beta, float eps, const float *z, int ldz,
                                       int offz, const float *local, int local_ld, float *out, float *stats, int B, int64_t hw,
                                       int C, void *stream) {
    FD_REQUIRE(y && gamma && beta && z && out && stats, "fd_ln_silu_gate_fwd_f32: null pointer");
    FD_REQUIRE(lsg_shape_ok(B, hw, C), "fd_ln_silu_gate_fwd_f32: unsupported shape B=%d hw=%lld C=%d (C %% 64 == 0, C <= 1024)", B,
               (long long)hw, C);
    FD_REQUIRE(ldz % 4 == 0 && offz % 4 == 0 && offz >= 0 && ldz >= offz + C && (!local || (local_ld % 4 == 0 && local_ld >= C)),
               "fd_ln_silu_gate_fwd_f32: strides / offsets must be multiples of 4 with off + C <= ld (ldz=%d offz=%d local_ld=%d)",
               ldz, offz, local_ld);
    FD_REQUIRE(al16(y) && al16(gamma) && al16(beta) && al16(z) && al16(local) && al16(out),
               "fd_ln_silu_gate_fwd_f32: tensors must be 16-byte aligned");
    const LsgPlan p = lsg_plan(B, hw, C);
    const int64_t nrows = (int64_t)B * hw;
    FD_LSG_VPL(lsg_fwd_kernel, dim3((unsigned)((nrows + p.rpb - 1) / p.rpb)), dim3(256), 0, (hipStream_t)stream, y, gamma, beta, eps,
               z, ldz, offz, local, local_ld, out, stats, hw, C, p.lpr, nrows);
    FD_LAUNCH_OK("fd_ln_silu_gate_fwd_f32");
    return FD_OK;
}

extern "C" int64_t fd_ln_silu_gate_bwd_ws_floats(int B, int64_t hw, int C) {
    if (!lsg_shape_ok(B, hw, C)) return 0;
    return lsg_plan(B, hw, C).total;
}

extern "C" int fd_ln_silu_gate_bwd_f32(const float *dout, const float *y, const float *stats, const float *gamma, const float *beta,
                                       const float *z, int ldz, int offz, float *dy, float *dz, int lddz, int offdz, float *dgamma,
                                       float *dbeta, float *dlocal, float *ws, int B, int64_t hw, int C, void *stream) {
    FD_REQUIRE(dout && y && stats && gamma && beta && z && dy && dz && dgamma && dbeta && ws, "fd_ln_silu_gate_bwd_f32: null pointer");
    FD_REQUIRE(lsg_shape_ok(B, hw, C), "fd_ln_silu_gate_bwd_f32: unsupported shape B=%d hw=%lld C=%d (C %% 64 == 0, C <= 1024)", B,
               (long long)hw, C);
    FD_REQUIRE(ldz % 4 == 0 && offz % 4 == 0 && offz >= 0 && ldz >= offz + C && lddz % 4 == 0 && offdz % 4 == 0 && offdz >= 0 &&
                   lddz >= offdz + C,
               "fd_ln_silu_gate_bwd_f32: strides / offsets must be multiples of 4 with off + C <= ld (ldz=%d offz=%d lddz=%d "
               "offdz=%d)", ldz, offz, lddz, offdz);
    FD_REQUIRE(al16(dout) && al16(y) && al16(gamma) && al16(beta) && al16(z) && al16(dy) && al16(dz) && al16(ws),
               "fd_ln_silu_gate_bwd_f32: tensors must be 16-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    const LsgPlan p = lsg_plan(B, hw, C);
    float *part = ws, *stage = part + p.part, *fin = stage + p.stage;
    FD_LSG_VPL(lsg_bwd_kernel, dim3((unsigned)p.nchunk, (unsigned)B), dim3(256), 0, st, dout, y, stats, gamma, beta, z, ldz, offz, dy,
               dz, lddz, offdz, part, hw, C, p.lpr, p.ch);
    const int64_t Q = 3 * (int64_t)C;
    launch_sum(part, Q, (int64_t)p.nchunk * Q, p.nchunk, (int)Q, LSG_G, stage, Q, (int64_t)p.M1 * Q, B, st);
    launch_sum(stage, Q, (int64_t)p.M1 * Q, p.M1, (int)Q, p.M1, fin, Q, Q, B, st);
    hipLaunchKernelGGL(lsg_finish_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, fin, B, C, dgamma, dbeta, dlocal);
    FD_LAUNCH_OK("fd_ln_silu_gate_bwd_f32");
    return FD_OK;
}
#undef FD_LSG_VPL
