// fd_tattn_train.hip -- the core of the reference's TransposedAttention (src/DADiff.py:252-285, Restormer channel attention)
// for training, fp32, NHWC, on the thirds q | k | v of qkv_dwconv's output qkv [B,hw,ld] in place.  Per (b, head), i and j over
// the head's 32 channels:
//
//   fd_chan_attn_fwd_f32   G = q^T k over all pixels, nq / nk the column norms (clamped at 1e-12 as F.normalize),
//                          Ghat = G / (nq nk^T), P = softmax_j(Ghat temperature[head]), out[p,i] = sum_j P[i][j] v[p,j]
//   fd_chan_attn_bwd_f32   dP = dout^T v, dS = P o (dP - rowsum(dP o P)), dtemperature = sum dS o Ghat, M = temperature dS,
//                          dq = (M khat - qhat rowsum(M o Ghat)) / nq, dk = (M^T qhat - khat colsum(M o Ghat)) / nk, dv = P^T dout
//
// The 32 x 32 attention never multiplies an [hw]-long normalised copy of q or k: the normalisation is folded into the small
// matrices.  Forward: a Gram pass (q, k in), its reduction, a per-(b, head) softmax kernel, one streaming pass (v in, out out).
// Backward: a Gram pass (dout, v in), its reduction, a per-(b, head) kernel in double precision that turns dP into
// Aq = M / (nq nk^T), cq = rowsum(M o Ghat) / nq^2, ck = colsum(M o Ghat) / nk^2, and one streaming pass
//      dq[p,i] = sum_j Aq[i][j] k[p,j] - cq[i] q[p,i],  dk[p,j] = sum_i Aq[i][j] q[p,i] - ck[j] k[p,j],  dv[p,j] = sum_i P[i][j] dout[p,i]
// that reads q, k, dout and writes the three thirds of dqkv: 6 x 128 bytes and 3 mat-vecs of 32 x 32 per pixel and head.
//
// The streaming passes run on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32) WITHOUT LDS: a wave owns 16 pixels of one head; lane
// (fr = lane & 15, fg = lane >> 4) loads the two 16-byte chunks [4 fg, +4) and [16 + 4 fg, +4) of pixel fr's 32 channels.  The
// MFMA's B operand wants element [k = fg][n = fr] per lane: element e of chunk t is taken as contraction index k of step (t, e),
// i.e. the contraction runs over the channels in the order 16 t + 4 fg + e -- a permutation that costs nothing because the A
// operand (the small matrix, 16 registers per product, loaded once per workgroup) is read in the same order.  The result tile
// [m = 4 fg + e][n = fr] is again 4 consecutive channels of pixel fr per lane: 16-byte stores, and the q / k values of the
// diagonal terms are the very registers the lane loaded.  48 MFMAs (1536 cycles) per 12 KB moved by a wave in the backward pass:
// the matrix pipe would keep up with ~19 TB/s, the pass is bound by HBM.
//
// Deterministic: Gram partials per pixel block in the workspace, summed in a fixed order; dtemperature summed over the batch in
// order; no float atomics.  The pixel-block size and every order of summation depend on hw only: a slice's results are the same
// bits alone or in a batch.  C % 64 == 0, C <= 512, heads of 32 channels.
#include "fd_train_common.h"

namespace {

constexpr int TA_LDP = 48;                 // LDS row stride of the Gram tiles (32 channels + pad)
constexpr int TA_SLOT = 1024 + 64;         // one Gram partial: 32 x 32 products, 32 + 32 sums of squares
constexpr int TA_ROWS = 256;               // pixels per workgroup of the streaming passes

// pixels per Gram block, the rule of fd_attn.hip: a function of the image size only
inline int ta_pb(int64_t hw) { return hw >= 65536 ? 1024 : 256; }
inline int ta_nblk(int64_t hw) { return (int)((hw + ta_pb(hw) - 1) / ta_pb(hw)); }
bool ta_shape_ok(int B, int64_t hw, int C) {
    return B > 0 && B < 65536 && hw > 0 && hw < (1ll << 31) && C > 0 && C % 64 == 0 && C <= 512 && (int64_t)B * (C / 32) < 65536;
}

// partial[b][head][blk] = (a^T bm over the block's pixels | column sums of squares of a | of bm); a, bm: pixel stride lda / ldb,
// channel offset offa / offb (the head's 32 channels follow)
__global__ __launch_bounds__(256) void ta_gram_kernel(const float *__restrict__ a, int lda, int offa, const float *__restrict__ bm,
                                                     int ldb, int offb, int64_t hw, int PB, float *__restrict__ partial, int nblk) {
    __shared__ __attribute__((aligned(16))) float sA[64 * TA_LDP], sB[64 * TA_LDP];
    __shared__ float sN[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int blk = blockIdx.x, head = blockIdx.y, b = blockIdx.z, heads = gridDim.y;
    const int pr = tid >> 2, cv = tid & 3;
    const int64_t p0 = (int64_t)blk * PB;
    const int64_t p1 = min(p0 + (int64_t)PB, hw);
    const float *pa = a + (int64_t)b * hw * lda + offa + head * 32 + cv * 8;
    const float *pb = bm + (int64_t)b * hw * ldb + offb + head * 32 + cv * 8;
    const int i0 = 16 * (wave >> 1), j0 = 16 * (wave & 1);
    const int fr = lane & 15, fg = lane >> 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float sa[8], sb[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) sa[e] = sb[e] = 0.f;
    for (int64_t pt = p0; pt < p1; pt += 64) {
        const int64_t p = pt + pr;
        float a8[8], b8[8];
        if (p < p1) {
            load8(pa + p * lda, a8);
            load8(pb + p * ldb, b8);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) a8[e] = b8[e] = 0.f;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            sa[e] += a8[e] * a8[e];
            sb[e] += b8[e] * b8[e];
            sA[pr * TA_LDP + cv * 8 + e] = a8[e];
            sB[pr * TA_LDP + cv * 8 + e] = b8[e];
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const float x = sA[(4 * s + fg) * TA_LDP + i0 + fr];
            const float y = sB[(4 * s + fg) * TA_LDP + j0 + fr];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x, y, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    float *out = partial + (((int64_t)b * heads + head) * nblk + blk) * TA_SLOT;
#pragma unroll
    for (int e = 0; e < 4; ++e) out[(i0 + fg * 4 + e) * 32 + j0 + fr] = acc[e];
    // sums of squares: lanes with equal (tid & 3) own the same 8 channels
#pragma unroll
    for (int e = 0; e < 8; ++e) {
#pragma unroll
        for (int o = 4; o < 64; o <<= 1) {
            sa[e] += __shfl_xor(sa[e], o, 64);
            sb[e] += __shfl_xor(sb[e], o, 64);
        }
    }
    if (lane < 4) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            sN[wave][lane * 8 + e] = sa[e];
            sN[wave][32 + lane * 8 + e] = sb[e];
        }
    }
    __syncthreads();
    if (tid < 64) out[1024 + tid] = (sN[0][tid] + sN[1][tid]) + (sN[2][tid] + sN[3][tid]);
}

// the pixel-block partials of one (b, head) summed in place into block 0's slot: a workgroup owns 64 of the 1088 entries, four
// thread groups take the blocks 4 apart, fixed order
__global__ __launch_bounds__(256) void ta_reduce_kernel(float *__restrict__ partial, int nblk) {
    __shared__ float sh[4][64];
    const int l = threadIdx.x & 63, col = blockIdx.x * 64 + l, grp = threadIdx.x >> 6;
    float *pp = partial + (int64_t)blockIdx.y * nblk * TA_SLOT;
    float s = 0.f;
    if (col < TA_SLOT) {
        int k = grp;
        for (; k + 12 < nblk; k += 16) {
            const float a0 = pp[(int64_t)k * TA_SLOT + col], a1 = pp[(int64_t)(k + 4) * TA_SLOT + col];
            const float a2 = pp[(int64_t)(k + 8) * TA_SLOT + col], a3 = pp[(int64_t)(k + 12) * TA_SLOT + col];
            s += (a0 + a1) + (a2 + a3);
        }
        for (; k < nblk; k += 4) s += pp[(int64_t)k * TA_SLOT + col];
    }
    sh[grp][l] = s;
    __syncthreads();
    if (grp == 0 && col < TA_SLOT) pp[col] = (sh[0][l] + sh[1][l]) + (sh[2][l] + sh[3][l]);
}

// grid (heads, B): the reduced Gram -> nrm (nq | nk), ghat, attn = softmax_j(ghat temperature)
__global__ __launch_bounds__(64) void ta_softmax_kernel(const float *__restrict__ partial, int nblk, const float *__restrict__ temperature,
                                                       float *__restrict__ attn, float *__restrict__ ghat, float *__restrict__ nrm) {
    __shared__ float sG[32 * 33], sP[32 * 33], sN[64];
    const int tid = threadIdx.x, head = blockIdx.x, heads = gridDim.x;
    const int64_t bh = (int64_t)blockIdx.y * heads + head;
    const float *pp = partial + bh * nblk * TA_SLOT;
    for (int i = tid; i < 1024; i += 64) sG[(i >> 5) * 33 + (i & 31)] = pp[i];
    {
        const float n = fmaxf(sqrtf(pp[1024 + tid]), 1e-12f);        // F.normalize's eps
        sN[tid] = n;
        nrm[bh * 64 + tid] = n;
    }
    __syncthreads();
    const float temp = temperature[head];
    if (tid < 32) {
        float mx = -3.4e38f;
        for (int j = 0; j < 32; ++j) {
            const float g = sG[tid * 33 + j] / (sN[tid] * sN[32 + j]);
            sG[tid * 33 + j] = g;
            mx = fmaxf(mx, g * temp);
        }
        float den = 0.f;
        for (int j = 0; j < 32; ++j) {
            const float e = expf(sG[tid * 33 + j] * temp - mx);
            sP[tid * 33 + j] = e;
            den += e;
        }
        for (int j = 0; j < 32; ++j) sP[tid * 33 + j] /= den;
    }
    __syncthreads();
    for (int i = tid; i < 1024; i += 64) {
        attn[bh * 1024 + i] = sP[(i >> 5) * 33 + (i & 31)];
        ghat[bh * 1024 + i] = sG[(i >> 5) * 33 + (i & 31)];
    }
}

// A operand of D[m][n] += sum_k A[m][k] B[k][n] for rows [16 blk, +16) of the 32 x 32 matrix mat (TR: of its transpose), the
// contraction index of step s = 4 t + e being channel 16 t + 4 fg + e
template <bool TR>
__device__ __forceinline__ void ta_load_a(const float *__restrict__ mat, int blk, int fr, int fg, float (&a)[8]) {
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int m = 16 * blk + fr, k = 16 * (s >> 2) + 4 * fg + (s & 3);
        a[s] = TR ? mat[k * 32 + m] : mat[m * 32 + k];
    }
}

__device__ __forceinline__ f32x4 ta_mm(const float (&a)[8], const f32x4 &x0, const f32x4 &x1, f32x4 acc) {
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], x0[e], acc, 0, 0, 0);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 + e], x1[e], acc, 0, 0, 0);
    return acc;
}

// grid (pixel chunk, head, b): out[p, i] = sum_j attn[i][j] v[p, j]
__global__ __launch_bounds__(256) void ta_apply_kernel(const float *__restrict__ v, int ld, int off, const float *__restrict__ attn,
                                                      float *__restrict__ out, int ldo, int64_t hw) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fg = lane >> 4;
    const int head = blockIdx.y, heads = gridDim.y;
    const int64_t b = blockIdx.z;
    const float *P = attn + (b * heads + head) * 1024;
    float a0[8], a1[8];
    ta_load_a<false>(P, 0, fr, fg, a0);
    ta_load_a<false>(P, 1, fr, fg, a1);
    const int64_t pbeg = (int64_t)blockIdx.x * TA_ROWS + wave * 16 + fr;
#pragma unroll 2
    for (int it = 0; it < TA_ROWS / 64; ++it) {
        const int64_t p = pbeg + it * 64;
        const bool ok = p < hw;
        f32x4 x0 = {0.f, 0.f, 0.f, 0.f}, x1 = x0;
        if (ok) {
            const float *src = v + (b * hw + p) * ld + off + head * 32 + 4 * fg;
            x0 = *(const f32x4 *)src;
            x1 = *(const f32x4 *)(src + 16);
        }
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        const f32x4 o0 = ta_mm(a0, x0, x1, z), o1 = ta_mm(a1, x0, x1, z);
        if (ok) {
            float *dst = out + (b * hw + p) * ldo + head * 32 + 4 * fg;
            *(f32x4 *)dst = o0;
            *(f32x4 *)(dst + 16) = o1;
        }
    }
}

// grid (heads, B), double precision: dP (the reduced Gram of dout and v), attn, ghat, nrm -> coef[b][head] = (Aq 32 x 32 | cq 32 |
// ck 32) and dtpart[b][head] = sum dS o ghat.
// one_pixel (hw == 1): a column normalised over a single pixel is sign(q), whose derivative is zero.  The general form reaches
// that zero only as the difference of two terms of size |M| / |q|, which fp32 does not resolve for a small |q|: the closed form
// Aq = cq = ck = 0 is written instead (dq = dk = 0; dv and dtemperature are not affected).
__global__ __launch_bounds__(64) void ta_bwd_small_kernel(const float *__restrict__ partial, int nblk, const float *__restrict__ temperature,
                                                         const float *__restrict__ attn, const float *__restrict__ ghat,
                                                         const float *__restrict__ nrm, float *__restrict__ coef,
                                                         float *__restrict__ dtpart, int one_pixel) {
    __shared__ double sM[32 * 33];
    __shared__ float sD[32 * 33], sP[32 * 33], sG[32 * 33], sN[64];
    __shared__ double sT[32], sRq[32], sRk[32];
    const int tid = threadIdx.x, head = blockIdx.x, heads = gridDim.x;
    const int64_t bh = (int64_t)blockIdx.y * heads + head;
    const float *pp = partial + bh * nblk * TA_SLOT;
    for (int i = tid; i < 1024; i += 64) {
        const int at = (i >> 5) * 33 + (i & 31);
        sD[at] = pp[i];
        sP[at] = attn[bh * 1024 + i];
        sG[at] = ghat[bh * 1024 + i];
    }
    sN[tid] = nrm[bh * 64 + tid];
    __syncthreads();
    const double temp = (double)temperature[head];
    if (tid < 32) {
        double row = 0.0, dt = 0.0, rq = 0.0;
        for (int j = 0; j < 32; ++j) row += (double)sD[tid * 33 + j] * (double)sP[tid * 33 + j];
        for (int j = 0; j < 32; ++j) {
            const double g = (double)sG[tid * 33 + j];
            const double ds = (double)sP[tid * 33 + j] * ((double)sD[tid * 33 + j] - row);
            const double m = temp * ds;
            dt += ds * g;
            rq += m * g;
            sM[tid * 33 + j] = m;
        }
        sT[tid] = dt;
        sRq[tid] = rq;
    }
    __syncthreads();
    if (tid < 32) {
        double rk = 0.0;
        for (int i = 0; i < 32; ++i) rk += sM[i * 33 + tid] * (double)sG[i * 33 + tid];
        sRk[tid] = rk;
    }
    __syncthreads();
    float *cf = coef + bh * TA_SLOT;
    for (int i = tid; i < 1024; i += 64) {
        const int r = i >> 5, c = i & 31;
        cf[i] = one_pixel ? 0.f : (float)(sM[r * 33 + c] / ((double)sN[r] * (double)sN[32 + c]));
    }
    {
        // a column whose norm sits at the clamp is divided by a constant: no second term (the gradient of x / eps)
        const double n = (double)sN[tid], r = tid < 32 ? sRq[tid] : sRk[tid - 32];
        cf[1024 + tid] = sN[tid] > 1e-12f && !one_pixel ? (float)(r / (n * n)) : 0.f;
    }
    if (tid == 0) {
        double t = 0.0;
        for (int i = 0; i < 32; ++i) t += sT[i];
        dtpart[bh] = (float)t;
    }
}

__global__ __launch_bounds__(64) void ta_dtemp_kernel(const float *__restrict__ dtpart, int B, int heads, float *__restrict__ dtemperature) {
    const int h = blockIdx.x * 64 + threadIdx.x;
    if (h >= heads) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += dtpart[(int64_t)b * heads + h];
    dtemperature[h] = s;
}

// grid (pixel chunk, head, b): the three thirds of dqkv from q, k, dout and the small matrices
__global__ __launch_bounds__(256) void ta_bwd_stream_kernel(const float *__restrict__ qkv, int ld, int off, const float *__restrict__ dout,
                                                           const float *__restrict__ attn, const float *__restrict__ coef,
                                                           float *__restrict__ dqkv, int ldd, int offd, int64_t hw, int C) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fg = lane >> 4;
    const int head = blockIdx.y, heads = gridDim.y;
    const int64_t b = blockIdx.z;
    const float *P = attn + (b * heads + head) * 1024;
    const float *cf = coef + (b * heads + head) * TA_SLOT;
    float av0[8], av1[8], aq0[8], aq1[8], ak0[8], ak1[8];
    ta_load_a<true>(P, 0, fr, fg, av0);          // dv^T = P^T dout^T
    ta_load_a<true>(P, 1, fr, fg, av1);
    ta_load_a<false>(cf, 0, fr, fg, aq0);        // dq^T = Aq k^T
    ta_load_a<false>(cf, 1, fr, fg, aq1);
    ta_load_a<true>(cf, 0, fr, fg, ak0);         // dk^T = Aq^T q^T
    ta_load_a<true>(cf, 1, fr, fg, ak1);
    const f32x4 cq0 = *(const f32x4 *)(cf + 1024 + 4 * fg), cq1 = *(const f32x4 *)(cf + 1024 + 16 + 4 * fg);
    const f32x4 ck0 = *(const f32x4 *)(cf + 1056 + 4 * fg), ck1 = *(const f32x4 *)(cf + 1056 + 16 + 4 * fg);
    const int64_t pbeg = (int64_t)blockIdx.x * TA_ROWS + wave * 16 + fr;
    for (int it = 0; it < TA_ROWS / 64; ++it) {
        const int64_t p = pbeg + it * 64;
        const bool ok = p < hw;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        f32x4 q0 = z, q1 = z, k0 = z, k1 = z, d0 = z, d1 = z;
        if (ok) {
            const float *src = qkv + (b * hw + p) * ld + off + head * 32 + 4 * fg;
            const float *sd = dout + (b * hw + p) * C + head * 32 + 4 * fg;
            q0 = *(const f32x4 *)src;
            q1 = *(const f32x4 *)(src + 16);
            k0 = *(const f32x4 *)(src + C);
            k1 = *(const f32x4 *)(src + C + 16);
            d0 = *(const f32x4 *)sd;
            d1 = *(const f32x4 *)(sd + 16);
        }
        const f32x4 dq0 = ta_mm(aq0, k0, k1, -(cq0 * q0)), dq1 = ta_mm(aq1, k0, k1, -(cq1 * q1));
        const f32x4 dk0 = ta_mm(ak0, q0, q1, -(ck0 * k0)), dk1 = ta_mm(ak1, q0, q1, -(ck1 * k1));
        const f32x4 dv0 = ta_mm(av0, d0, d1, z), dv1 = ta_mm(av1, d0, d1, z);
        if (ok) {
            float *dst = dqkv + (b * hw + p) * ldd + offd + head * 32 + 4 * fg;
            *(f32x4 *)dst = dq0;
            *(f32x4 *)(dst + 16) = dq1;
            *(f32x4 *)(dst + C) = dk0;
            *(f32x4 *)(dst + C + 16) = dk1;
            *(f32x4 *)(dst + 2 * C) = dv0;
            *(f32x4 *)(dst + 2 * C + 16) = dv1;
        }
    }
}

void ta_gram(const float *a, int lda, int offa, const float *bm, int ldb, int offb, float *partial, int B, int64_t hw, int C,
             hipStream_t st) {
    const int nblk = ta_nblk(hw), heads = C / 32;
    hipLaunchKernelGGL(ta_gram_kernel, dim3((unsigned)nblk, (unsigned)heads, (unsigned)B), dim3(256), 0, st, a, lda, offa, bm, ldb,
                       offb, hw, ta_pb(hw), partial, nblk);
    if (nblk > 1)
        hipLaunchKernelGGL(ta_reduce_kernel, dim3(17, (unsigned)(B * heads)), dim3(256), 0, st, partial, nblk);
}

}  // namespace

extern "C" int64_t fd_chan_attn_fwd_ws_floats(int B, int64_t hw, int C) {
    if (!ta_shape_ok(B, hw, C)) return 0;
    return round4((int64_t)B * (C / 32) * ta_nblk(hw) * TA_SLOT);
}

extern "C" int fd_chan_attn_fwd_f32(const float *qkv, int ld, int off, const float *temperature, float *out, float *attn,
                                    float *ghat, float *nrm, float *ws, int B, int64_t hw, int C, void *stream) {
    FD_REQUIRE(qkv && temperature && out && attn && ghat && nrm && ws, "fd_chan_attn_fwd_f32: null pointer");
    FD_REQUIRE(ta_shape_ok(B, hw, C), "fd_chan_attn_fwd_f32: unsupported shape B=%d hw=%lld C=%d (C %% 64 == 0, C <= 512)", B,
               (long long)hw, C);
    FD_REQUIRE(ld % 4 == 0 && off % 4 == 0 && off >= 0 && ld >= off + 3 * C,
               "fd_chan_attn_fwd_f32: stride / offset must be multiples of 4 with off + 3 C <= ld (ld=%d off=%d C=%d)", ld, off, C);
    FD_REQUIRE(al16(qkv) && al16(out) && al16(ws), "fd_chan_attn_fwd_f32: tensors must be 16-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    const int heads = C / 32;
    ta_gram(qkv, ld, off, qkv, ld, off + C, ws, B, hw, C, st);
    hipLaunchKernelGGL(ta_softmax_kernel, dim3((unsigned)heads, (unsigned)B), dim3(64), 0, st, ws, ta_nblk(hw), temperature, attn,
                       ghat, nrm);
    hipLaunchKernelGGL(ta_apply_kernel, dim3((unsigned)((hw + TA_ROWS - 1) / TA_ROWS), (unsigned)heads, (unsigned)B), dim3(256), 0, st,
                       qkv, ld, off + 2 * C, attn, out, C, hw);
    FD_LAUNCH_OK("fd_chan_attn_fwd_f32");
    return FD_OK;
}

extern "C" int64_t fd_chan_attn_bwd_ws_floats(int B, int64_t hw, int C) {
    if (!ta_shape_ok(B, hw, C)) return 0;
    const int64_t bh = (int64_t)B * (C / 32);
    return round4(bh * ta_nblk(hw) * TA_SLOT) + round4(bh * TA_SLOT) + round4(bh);
}

extern "C" int fd_chan_attn_bwd_f32(const float *qkv, int ld, int off, const float *temperature, const float *attn,
                                    const float *ghat, const float *nrm, const float *dout, float *dqkv, int ld_d, int off_d,
                                    float *dtemperature, float *ws, int B, int64_t hw, int C, void *stream) {
    FD_REQUIRE(qkv && temperature && attn && ghat && nrm && dout && dqkv && dtemperature && ws, "fd_chan_attn_bwd_f32: null pointer");
    FD_REQUIRE(ta_shape_ok(B, hw, C), "fd_chan_attn_bwd_f32: unsupported shape B=%d hw=%lld C=%d (C %% 64 == 0, C <= 512)", B,
               (long long)hw, C);
    FD_REQUIRE(ld % 4 == 0 && off % 4 == 0 && off >= 0 && ld >= off + 3 * C && ld_d % 4 == 0 && off_d % 4 == 0 && off_d >= 0 &&
                   ld_d >= off_d + 3 * C,
               "fd_chan_attn_bwd_f32: strides / offsets must be multiples of 4 with off + 3 C <= ld (ld=%d off=%d ld_d=%d off_d=%d "
               "C=%d)", ld, off, ld_d, off_d, C);
    FD_REQUIRE(al16(qkv) && al16(dout) && al16(dqkv) && al16(ws), "fd_chan_attn_bwd_f32: tensors must be 16-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    const int heads = C / 32;
    const int64_t bh = (int64_t)B * heads;
    float *partial = ws, *coef = partial + round4(bh * ta_nblk(hw) * TA_SLOT), *dtpart = coef + round4(bh * TA_SLOT);
    ta_gram(dout, C, 0, qkv, ld, off + 2 * C, partial, B, hw, C, st);
    hipLaunchKernelGGL(ta_bwd_small_kernel, dim3((unsigned)heads, (unsigned)B), dim3(64), 0, st, partial, ta_nblk(hw), temperature,
                       attn, ghat, nrm, coef, dtpart, hw == 1 ? 1 : 0);
    hipLaunchKernelGGL(ta_dtemp_kernel, dim3((unsigned)((heads + 63) / 64)), dim3(64), 0, st, dtpart, B, heads, dtemperature);
    hipLaunchKernelGGL(ta_bwd_stream_kernel, dim3((unsigned)((hw + TA_ROWS - 1) / TA_ROWS), (unsigned)heads, (unsigned)B), dim3(256), 0,
                       st, qkv, ld, off, dout, attn, coef, dqkv, ld_d, off_d, hw, C);
    FD_LAUNCH_OK("fd_chan_attn_bwd_f32");
    return FD_OK;
}
