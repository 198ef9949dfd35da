// fd_train_crop.hip -- a training batch of patches straight from a slice store on the device: the reference's CropToFixed
// (data/transforms.py:196-249) in front of the RandomFlip + RandomRotate90 of fd_train_data.hip, in the same one launch:
//
//   fd_store_crop_f32         x_start, x_input = the cropped, transformed pair of every item: a copy
//   fd_res_qsample_crop_f32   what fd_res_qsample_f32 (fd_train_step.hip) does to that batch, without assembling it
//
// Item b is cut to the CH x CW window at (y0, x0) = windows[b] of its H x W slices; an axis no longer than the crop is taken whole
// and reflect-padded to it ((c - n) / 2 in front, the rest behind; no edge repeat, one reflection).  The code of fd_train_data.hip
// then applies to the crop: with (ic, jc) the crop pixel src_map gives for output pixel (y, x), the source pixel is
// (refl(y0 - pad_top + ic, H), refl(x0 - pad_left + jc, W)), refl(v, n) = -v below 0, 2 (n - 1) - v from n on.  The forms are those of
// store_batch_kernel, chosen per blockIdx.y:
//   direct (k even)  every lane owns 4 consecutive output pixels of one crop row (CW % 4 == 0) and reads 4 consecutive source
//                    pixels, reversed in registers under a W flip
//   tiled (k odd)    a workgroup owns a 64 x 64 output tile of both images and turns it through float[64][65] per image in the LDS
//   per pixel        CW % 4 != 0 or an output pointer (or the given noise) is not 16-byte aligned: the same ownership, every form
// The four source pixels of a group start at column x0 + ..., which is 4-byte aligned and no more.  They are read through f32x4_a4,
// a vector type that promises only that: hipcc turns it into one global_load_dwordx4, which the hardware accepts at any dword
// address (checked in the ISA and for every x0 % 4 in tests/test_gpu_train_crop.py); a cast to f32x4 would promise 16 bytes.  A
// group that touches the reflect padding reads pixel by pixel.  The stores and the noise are in output order and stay 16-byte.
// The arithmetic and the noise are emit4's (fd_train_batch.h): output pixel p of the crop takes element p % 4 of
// keyed_normal4(seed, step, p / 4), so the fused entry gives the bits of fd_store_crop_f32 followed by fd_res_qsample_f32.  No
// atomics, nothing synchronises with the host.  The slots are clamped to the store, the window to [0, max(H - CH, 0)] x
// [0, max(W - CW, 0)], every reflected coordinate to its axis, and an odd k on a non-square crop is dropped: no argument reads
// outside the store.  All source addressing is int64.
#include "fd_train_batch.h"

namespace {

struct CropArgs {
    BatchArgs b;                       // H, W: the store's slices; every output is B x CH x CW
    const int64_t *windows;            // (B, 2) = y0, x0 per item; null: (0, 0)
    int CH, CW;
};

typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ int refl(int v, int n) {
    v = v < 0 ? -v : v;
    v = v >= n ? 2 * (n - 1) - v : v;
    return min(max(v, 0), n - 1);      // a second reflection never happens (the entries check the pads); out of range stays inside
}

// q[e] = crop pixel (., jc + e), e < 4, of the source row rp; ox: the source column of crop column 0
__device__ __forceinline__ void row4(const float *rp, int ox, int jc, int W, float q[4]) {
    const int cl = ox + jc;
    if (cl >= 0 && cl + 3 < W) {
        const f32x4_a4 v = *(const f32x4_a4 *)(rp + cl);
        q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] = rp[refl(cl + e, W)];
    }
}

// grid (max(groups of four pixels / 256, 64 x 64 tiles), b).  VEC: CW % 4 == 0 and every pointer in output order 16-byte aligned.
template <bool VEC, int MODE>
__global__ __launch_bounds__(256) void crop_batch_kernel(const CropArgs c) {
    __shared__ float s0[VEC ? TD_TILE * TD_PITCH : 1], si[VEC ? TD_TILE * TD_PITCH : 1];
    const BatchArgs &a = c.b;
    const int b = blockIdx.y, tid = threadIdx.x, H = a.H, W = a.W, CH = c.CH, CW = c.CW;
    float ac = 0.f, bc = 0.f;
    if (MODE != MODE_GATHER) {
        const int64_t tb = min(max(a.t[b], (int64_t)0), (int64_t)a.T - 1);   // a timestep outside the table reads its nearest row
        ac = a.acs[tb];
        bc = a.bcs[tb];
        if (blockIdx.x == 0 && tid == 0) {
            a.times[b] = ac * (float)a.T;
            a.times[a.B + b] = bc * (float)a.T;
        }
    }
    const int64_t npix = (int64_t)CH * CW, spix = (int64_t)H * W;
    const float *pn = a.nd + min(max(a.nd_slot[b], (int64_t)0), a.n_nd - 1) * spix;
    const float *pl = a.ld + min(max(a.ld_slot[b], (int64_t)0), a.n_ld - 1) * spix;
    const SrcMap m = src_map(a.codes ? (int)(a.codes[b] & 15) : 0, CH == CW);
    int wy = 0, wx = 0;
    if (c.windows) {
        wy = (int)min(max(c.windows[2 * b], (int64_t)0), (int64_t)max(H - CH, 0));
        wx = (int)min(max(c.windows[2 * b + 1], (int64_t)0), (int64_t)max(W - CW, 0));
    }
    const int oy = wy - (CH > H ? (CH - H) / 2 : 0), ox = wx - (CW > W ? (CW - W) / 2 : 0);   // the source of crop pixel (0, 0)
    float v0[4], vi[4], qn[4], ql[4];
    if (VEC && m.tr) {                                                   // the same for every lane of the workgroup; CH == CW
        const int tiles_x = (CW + TD_TILE - 1) / TD_TILE, tiles_y = (CH + TD_TILE - 1) / TD_TILE;
        if ((int)blockIdx.x >= tiles_x * tiles_y) return;
        const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
        const int y0 = ty * TD_TILE, x0 = tx * TD_TILE;
        const int cc = tid & 7, r = tid >> 3;                            // 8 groups of four x 32 rows per pass
        // output pixels (y0 + ly4 ... + 3, x0 + lx) are crop pixels (ic, jc ... + 3) of one row, reversed under fj: to s[lx][ly4 ...]
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const int lx = r + 32 * (pass >> 1), ly4 = 4 * cc + 32 * (pass & 1);
            const int x = x0 + lx, y = y0 + ly4;
            if (x < CW && y < CH) {
                const int ic = m.fi ? CH - 1 - x : x, jc = m.fj ? CW - 4 - y : y;
                const int64_t ro = (int64_t)refl(oy + ic, H) * W;
                row4(pn + ro, ox, jc, W, qn);
                row4(pl + ro, ox, jc, W, ql);
                float *d0 = s0 + lx * TD_PITCH + ly4, *di = si + lx * TD_PITCH + ly4;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int ee = m.fj ? 3 - e : e;
                    d0[ee] = qn[e];
                    di[ee] = ql[e];
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const int lx4 = 4 * cc + 32 * (pass & 1), ly = r + 32 * (pass >> 1);
            const int x = x0 + lx4, y = y0 + ly;
            if (x < CW && y < CH) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v0[e] = s0[(lx4 + e) * TD_PITCH + ly];
                    vi[e] = si[(lx4 + e) * TD_PITCH + ly];
                }
                emit4<true, MODE>(a, b, npix, (int64_t)y * CW + x, 4, v0, vi, ac, bc);
            }
        }
        return;
    }
    const int64_t i0 = 4 * ((int64_t)blockIdx.x * 256 + tid);
    if (i0 >= npix) return;
    const int n = (int)min((int64_t)4, npix - i0);
    int y = (int)((uint32_t)i0 / (uint32_t)CW), x = (int)((uint32_t)i0 - (uint32_t)y * (uint32_t)CW);    // npix <= 2^30
    if (VEC) {
        const int ic = m.fi ? CH - 1 - y : y, jc = m.fj ? CW - 4 - x : x;
        const int64_t ro = (int64_t)refl(oy + ic, H) * W;
        row4(pn + ro, ox, jc, W, qn);
        row4(pl + ro, ox, jc, W, ql);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v0[e] = m.fj ? qn[3 - e] : qn[e];
            vi[e] = m.fj ? ql[3 - e] : ql[e];
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v0[e] = vi[e] = 0.f;
            if (e < n) {
                const int p = m.tr ? x : y, q = m.tr ? y : x;
                const int ic = m.fi ? CH - 1 - p : p, jc = m.fj ? CW - 1 - q : q;
                const int64_t so = (int64_t)refl(oy + ic, H) * W + refl(ox + jc, W);
                v0[e] = pn[so];
                vi[e] = pl[so];
                if (++x == CW) {
                    x = 0;
                    ++y;
                }
            }
        }
    }
    emit4<VEC, MODE>(a, b, npix, i0, n, v0, vi, ac, bc);
}

// the larger pad of an axis of length n cropped to c is behind it
bool pad_ok(int n, int c) { return c <= n || (c - n) - (c - n) / 2 <= n - 1; }

bool crop_shape_ok(const CropArgs &c) {
    const BatchArgs &a = c.b;
    return a.B > 0 && a.B <= 65535 && a.H > 0 && a.H <= 32768 && a.W > 0 && a.W <= 32768 && c.CH > 0 && c.CH <= 32768 && c.CW > 0 &&
           c.CW <= 32768 && a.n_nd > 0 && a.n_ld > 0 && pad_ok(a.H, c.CH) && pad_ok(a.W, c.CW);
}

template <int MODE>
void crop_launch(const CropArgs &c, bool vec, hipStream_t st) {
    const int64_t npix = (int64_t)c.CH * c.CW;
    int64_t gx = ((npix + 3) / 4 + 255) / 256;
    if (vec) {                                                           // a slice with an odd k takes one workgroup per tile
        const int64_t tiles = (int64_t)((c.CW + TD_TILE - 1) / TD_TILE) * ((c.CH + TD_TILE - 1) / TD_TILE);
        if (tiles > gx) gx = tiles;
    }
    const dim3 grid((unsigned)gx, (unsigned)c.b.B);
    if (vec) hipLaunchKernelGGL((crop_batch_kernel<true, MODE>), grid, dim3(256), 0, st, c);
    else hipLaunchKernelGGL((crop_batch_kernel<false, MODE>), grid, dim3(256), 0, st, c);
}

}  // namespace

extern "C" int fd_store_crop_f32(const float *nd, const float *ld, int64_t n_nd, int64_t n_ld, const int64_t *nd_slot,
                                 const int64_t *ld_slot, const int64_t *codes, const int64_t *windows, float *x_start, float *x_input,
                                 int B, int H, int W, int CH, int CW, void *stream) {
    FD_REQUIRE(nd && ld && nd_slot && ld_slot && x_start && x_input, "fd_store_crop_f32: null pointer");
    CropArgs c = {};
    BatchArgs &a = c.b;
    a.nd = nd; a.ld = ld; a.n_nd = n_nd; a.n_ld = n_ld;
    a.nd_slot = nd_slot; a.ld_slot = ld_slot; a.codes = codes;
    a.B = B; a.H = H; a.W = W;
    a.x_start = x_start; a.x_input = x_input;
    c.windows = windows; c.CH = CH; c.CW = CW;
    FD_REQUIRE(crop_shape_ok(c),
               "fd_store_crop_f32: unsupported shape B=%d H=%d W=%d CH=%d CW=%d n_nd=%lld n_ld=%lld (B <= 65535, H, W, CH, CW <= 32768, "
               "a reflect pad of at most H - 1 / W - 1)", B, H, W, CH, CW, (long long)n_nd, (long long)n_ld);
    const bool vec = CW % 4 == 0 && al16(x_start) && al16(x_input);
    crop_launch<MODE_GATHER>(c, vec, (hipStream_t)stream);
    FD_LAUNCH_OK("fd_store_crop_f32");
    return FD_OK;
}

extern "C" int fd_res_qsample_crop_f32(const float *nd, const float *ld, int64_t n_nd, int64_t n_ld, const int64_t *nd_slot,
                                       const int64_t *ld_slot, const int64_t *codes, const int64_t *windows, const int64_t *t,
                                       const float *alphas_cumsum, const float *betas_cumsum, int T, const float *noise,
                                       const int64_t *seeds, int noise_step, int normalize, float *x_in, float *x_res,
                                       float *noise_out, float *times, float *x0, int B, int H, int W, int CH, int CW, void *stream) {
    FD_REQUIRE(nd && ld && nd_slot && ld_slot && t && alphas_cumsum && betas_cumsum && x_in && x_res && times,
               "fd_res_qsample_crop_f32: null pointer");
    FD_REQUIRE((noise != nullptr) != (seeds != nullptr), "fd_res_qsample_crop_f32: give either noise or seeds");
    FD_REQUIRE(!seeds || noise_out, "fd_res_qsample_crop_f32: seeds need a noise_out");
    CropArgs c = {};
    BatchArgs &a = c.b;
    a.nd = nd; a.ld = ld; a.n_nd = n_nd; a.n_ld = n_ld;
    a.nd_slot = nd_slot; a.ld_slot = ld_slot; a.codes = codes;
    a.B = B; a.H = H; a.W = W;
    a.t = t; a.acs = alphas_cumsum; a.bcs = betas_cumsum; a.T = T;
    a.noise = noise; a.seeds = seeds; a.noise_step = noise_step; a.normalize = normalize;
    a.x_in = x_in; a.x_res = x_res; a.noise_out = noise_out; a.times = times; a.x0 = x0;
    c.windows = windows; c.CH = CH; c.CW = CW;
    FD_REQUIRE(crop_shape_ok(c) && T > 0,
               "fd_res_qsample_crop_f32: unsupported shape B=%d H=%d W=%d CH=%d CW=%d T=%d n_nd=%lld n_ld=%lld (B <= 65535, H, W, CH, CW "
               "<= 32768, a reflect pad of at most H - 1 / W - 1)", B, H, W, CH, CW, T, (long long)n_nd, (long long)n_ld);
    const bool vec = CW % 4 == 0 && al16(noise) && al16(x_in) && al16(x_res) && al16(noise_out) && al16(x0);
    if (seeds) crop_launch<MODE_KEYED>(c, vec, (hipStream_t)stream);
    else crop_launch<MODE_NOISE>(c, vec, (hipStream_t)stream);
    FD_LAUNCH_OK("fd_res_qsample_crop_f32");
    return FD_OK;
}
