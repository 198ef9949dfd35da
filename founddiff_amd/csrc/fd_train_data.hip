// fd_train_data.hip -- a training batch straight from a slice store on the device, under the reference's RandomFlip +
// RandomRotate90 (data/pdf_dataset.py:521-545, data/transforms.py:25-82: one random state for the pair, so both images get the same
// transform):
//
//   fd_store_gather_f32        x_start, x_input = the two transformed images of every item: a copy
//   fd_res_qsample_store_f32   what fd_res_qsample_f32 (fd_train_step.hip) does to that batch, without assembling it
//
// A slice's code: bit 0 flips H, bit 1 flips W, bits 2-3 = k; out = rot90(flip_W(flip_H(m)), k).  src_map / src_offset (fd_train_batch.h)
// turn it into the source pixel of an output pixel, for both entries and both forms:
//   direct (k even)  every lane owns 4 consecutive output pixels and reads 4 consecutive source pixels, reversed in registers under
//                    a W flip; 16-byte accesses when W % 4 == 0 and every pointer is aligned, per pixel with the same ownership
//                    otherwise (then for odd k too)
//   tiled (k odd)    a workgroup owns a 64 x 64 output tile of both images: the source tile is read along its rows into
//                    float[64][65] per image in the LDS, read back along its columns and written along the output's rows.  With the
//                    65-dword pitch the 32 lanes of a half wave (8 groups of four x 4 rows) fall into 32 different banks on both
//                    sides.
// The code belongs to the slice, so the form is chosen per blockIdx.y; the grid is wide enough for either.  The arithmetic and the
// noise are qsample_kernel's: the same fmaf sequence, and output pixel p takes element p % 4 of keyed_normal4(seed, step, p / 4), so
// the fused entry gives the bits of the gather followed by fd_res_qsample_f32.  No atomics, nothing synchronises with the host.
// The slots are clamped to the store and an odd k on a non-square store is dropped: no argument reads outside the store.
#include "fd_train_batch.h"

namespace {

// grid (max(groups of four pixels / 256, 64 x 64 tiles), b).  VEC: W % 4 == 0 and every pointer 16-byte aligned.
template <bool VEC, int MODE>
__global__ __launch_bounds__(256) void store_batch_kernel(const BatchArgs a) {
    __shared__ float s0[VEC ? TD_TILE * TD_PITCH : 1], si[VEC ? TD_TILE * TD_PITCH : 1];
    const int b = blockIdx.y, tid = threadIdx.x, H = a.H, W = a.W;
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
    const int64_t npix = (int64_t)H * W;
    const float *pn = a.nd + min(max(a.nd_slot[b], (int64_t)0), a.n_nd - 1) * npix;
    const float *pl = a.ld + min(max(a.ld_slot[b], (int64_t)0), a.n_ld - 1) * npix;
    const SrcMap m = src_map(a.codes ? (int)(a.codes[b] & 15) : 0, H == W);
    float v0[4], vi[4];
    if (VEC && m.tr) {                                                   // the same for every lane of the workgroup
        const int tiles_x = (W + TD_TILE - 1) / TD_TILE, tiles_y = (H + TD_TILE - 1) / TD_TILE;
        if ((int)blockIdx.x >= tiles_x * tiles_y) return;
        const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
        const int y0 = ty * TD_TILE, x0 = tx * TD_TILE;
        const int c = tid & 7, r = tid >> 3;                             // 8 groups of four x 32 rows per pass
        // output pixels (y0 + ly4 ... + 3, x0 + lx) have consecutive sources: one 16-byte read, to s[lx][ly4 ...]
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const int lx = r + 32 * (pass >> 1), ly4 = 4 * c + 32 * (pass & 1);
            const int x = x0 + lx, y = y0 + ly4;
            if (x < W && y < H) {
                const int64_t so = src_offset(m, m.fj ? y + 3 : y, x, H, W);
                const f32x4 qn = *(const f32x4 *)(pn + so), ql = *(const f32x4 *)(pl + so);
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
            const int lx4 = 4 * c + 32 * (pass & 1), ly = r + 32 * (pass >> 1);
            const int x = x0 + lx4, y = y0 + ly;
            if (x < W && y < H) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v0[e] = s0[(lx4 + e) * TD_PITCH + ly];
                    vi[e] = si[(lx4 + e) * TD_PITCH + ly];
                }
                emit4<true, MODE>(a, b, npix, (int64_t)y * W + x, 4, v0, vi, ac, bc);
            }
        }
        return;
    }
    const int64_t i0 = 4 * ((int64_t)blockIdx.x * 256 + tid);
    if (i0 >= npix) return;
    const int n = (int)min((int64_t)4, npix - i0);
    int y = (int)((uint32_t)i0 / (uint32_t)W), x = (int)((uint32_t)i0 - (uint32_t)y * (uint32_t)W);      // npix <= 2^30
    if (VEC) {
        const int64_t so = src_offset(m, y, m.fj ? x + 3 : x, H, W);
        load4<true>(pn + so, 4, v0);
        load4<true>(pl + so, 4, vi);
        if (m.fj) {
            float s;
            s = v0[0]; v0[0] = v0[3]; v0[3] = s;
            s = v0[1]; v0[1] = v0[2]; v0[2] = s;
            s = vi[0]; vi[0] = vi[3]; vi[3] = s;
            s = vi[1]; vi[1] = vi[2]; vi[2] = s;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v0[e] = vi[e] = 0.f;
            if (e < n) {
                const int64_t so = src_offset(m, y, x, H, W);
                v0[e] = pn[so];
                vi[e] = pl[so];
                if (++x == W) {
                    x = 0;
                    ++y;
                }
            }
        }
    }
    emit4<VEC, MODE>(a, b, npix, i0, n, v0, vi, ac, bc);
}

bool store_shape_ok(const BatchArgs &a) {
    return a.B > 0 && a.B <= 65535 && a.H > 0 && a.H <= 32768 && a.W > 0 && a.W <= 32768 && a.n_nd > 0 && a.n_ld > 0;
}

template <int MODE>
void store_launch(const BatchArgs &a, bool vec, hipStream_t st) {
    const int64_t npix = (int64_t)a.H * a.W;
    int64_t gx = ((npix + 3) / 4 + 255) / 256;
    if (vec) {                                                           // a slice with an odd k takes one workgroup per tile
        const int64_t tiles = (int64_t)((a.W + TD_TILE - 1) / TD_TILE) * ((a.H + TD_TILE - 1) / TD_TILE);
        if (tiles > gx) gx = tiles;
    }
    const dim3 grid((unsigned)gx, (unsigned)a.B);
    if (vec) hipLaunchKernelGGL((store_batch_kernel<true, MODE>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((store_batch_kernel<false, MODE>), grid, dim3(256), 0, st, a);
}

}  // namespace

extern "C" int fd_store_gather_f32(const float *nd, const float *ld, int64_t n_nd, int64_t n_ld, const int64_t *nd_slot,
                                   const int64_t *ld_slot, const int64_t *codes, float *x_start, float *x_input, int B, int H, int W,
                                   void *stream) {
    FD_REQUIRE(nd && ld && nd_slot && ld_slot && x_start && x_input, "fd_store_gather_f32: null pointer");
    BatchArgs a = {};
    a.nd = nd; a.ld = ld; a.n_nd = n_nd; a.n_ld = n_ld;
    a.nd_slot = nd_slot; a.ld_slot = ld_slot; a.codes = codes;
    a.B = B; a.H = H; a.W = W;
    a.x_start = x_start; a.x_input = x_input;
    FD_REQUIRE(store_shape_ok(a), "fd_store_gather_f32: unsupported shape B=%d H=%d W=%d n_nd=%lld n_ld=%lld (B <= 65535, H, W <= 32768)",
               B, H, W, (long long)n_nd, (long long)n_ld);
    const bool vec = W % 4 == 0 && al16(nd) && al16(ld) && al16(x_start) && al16(x_input);
    store_launch<MODE_GATHER>(a, vec, (hipStream_t)stream);
    FD_LAUNCH_OK("fd_store_gather_f32");
    return FD_OK;
}

extern "C" int fd_res_qsample_store_f32(const float *nd, const float *ld, int64_t n_nd, int64_t n_ld, const int64_t *nd_slot,
                                        const int64_t *ld_slot, const int64_t *codes, const int64_t *t, const float *alphas_cumsum,
                                        const float *betas_cumsum, int T, const float *noise, const int64_t *seeds, int noise_step,
                                        int normalize, float *x_in, float *x_res, float *noise_out, float *times, float *x0, int B,
                                        int H, int W, void *stream) {
    FD_REQUIRE(nd && ld && nd_slot && ld_slot && t && alphas_cumsum && betas_cumsum && x_in && x_res && times,
               "fd_res_qsample_store_f32: null pointer");
    FD_REQUIRE((noise != nullptr) != (seeds != nullptr), "fd_res_qsample_store_f32: give either noise or seeds");
    FD_REQUIRE(!seeds || noise_out, "fd_res_qsample_store_f32: seeds need a noise_out");
    BatchArgs a = {};
    a.nd = nd; a.ld = ld; a.n_nd = n_nd; a.n_ld = n_ld;
    a.nd_slot = nd_slot; a.ld_slot = ld_slot; a.codes = codes;
    a.B = B; a.H = H; a.W = W;
    a.t = t; a.acs = alphas_cumsum; a.bcs = betas_cumsum; a.T = T;
    a.noise = noise; a.seeds = seeds; a.noise_step = noise_step; a.normalize = normalize;
    a.x_in = x_in; a.x_res = x_res; a.noise_out = noise_out; a.times = times; a.x0 = x0;
    FD_REQUIRE(store_shape_ok(a) && T > 0,
               "fd_res_qsample_store_f32: unsupported shape B=%d H=%d W=%d T=%d n_nd=%lld n_ld=%lld (B <= 65535, H, W <= 32768)", B, H, W,
               T, (long long)n_nd, (long long)n_ld);
    const bool vec = W % 4 == 0 && al16(nd) && al16(ld) && al16(noise) && al16(x_in) && al16(x_res) && al16(noise_out) && al16(x0);
    if (seeds) store_launch<MODE_KEYED>(a, vec, (hipStream_t)stream);
    else store_launch<MODE_NOISE>(a, vec, (hipStream_t)stream);
    FD_LAUNCH_OK("fd_res_qsample_store_f32");
    return FD_OK;
}
