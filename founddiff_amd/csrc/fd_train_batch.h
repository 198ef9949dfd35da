// fd_train_batch.h -- what the two files that make a training batch from a slice store share (fd_train_data.hip: whole slices,
// fd_train_crop.hip: crops): the flip / rot90 code as a source-pixel map, the arguments of a batch, and the arithmetic of
// qsample_kernel (fd_train_step.hip) on four output pixels.  Everything sits in an anonymous namespace, as in fd_train_common.h.
#pragma once
#include "fd_train_common.h"
#include "fd_keyed_noise.h"

namespace {

constexpr int TD_TILE = 64, TD_PITCH = 65;

struct SrcMap {
    bool tr, fi, fj;      // (i, j) = (F_i(tr ? x : y), F_j(tr ? y : x)), F a mirror where its flag is up
};

// k = 0: (y, x); 1: (x, W-1-y); 2: (H-1-y, W-1-x); 3: (H-1-x, y); then j = W-1-j if bit 1 and i = H-1-i if bit 0
__device__ __forceinline__ SrcMap src_map(int code, bool square) {
    int k = (code >> 2) & 3;
    if (!square) k &= 2;
    SrcMap m;
    m.tr = (k & 1) != 0;
    m.fi = (((k >> 1) ^ code) & 1) != 0;
    m.fj = (((k >> 1) ^ k ^ (code >> 1)) & 1) != 0;
    return m;
}

// the offset in its slice of the source pixel of output pixel (y, x)
__device__ __forceinline__ int64_t src_offset(const SrcMap &m, int y, int x, int H, int W) {
    const int a = m.tr ? x : y, b = m.tr ? y : x;
    const int i = m.fi ? H - 1 - a : a, j = m.fj ? W - 1 - b : b;
    return (int64_t)i * W + j;
}

struct BatchArgs {
    const float *nd, *ld;
    int64_t n_nd, n_ld;
    const int64_t *nd_slot, *ld_slot, *codes;
    int B, H, W;
    // the gather's outputs
    float *x_start, *x_input;
    // q_sample
    const int64_t *t;
    const float *acs, *bcs;
    int T;
    const float *noise;
    const int64_t *seeds;
    int noise_step, normalize;
    float *x_in, *x_res, *noise_out, *times, *x0;
};

constexpr int MODE_GATHER = 0, MODE_NOISE = 1, MODE_KEYED = 2;

// the four output pixels from i0 (a multiple of 4) of slice b, their sources in v0 (x_start) and vi (x_input)
template <bool VEC, int MODE>
__device__ __forceinline__ void emit4(const BatchArgs &a, int b, int64_t npix, int64_t i0, int n, float v0[4], float vi[4], float ac,
                                      float bc) {
    const int64_t row = (int64_t)b * npix + i0;
    if (MODE == MODE_GATHER) {
        store4<VEC>(a.x_start + row, n, v0);
        store4<VEC>(a.x_input + row, n, vi);
        return;
    }
    float z[4], xt[4], xr[4];
    if (MODE == MODE_KEYED) keyed_normal4((uint64_t)a.seeds[b], (uint32_t)a.noise_step, (uint32_t)(i0 >> 2), z);
    else load4<VEC>(a.noise + row, n, z);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (a.normalize) {
            v0[e] = fmaf(2.f, v0[e], -1.f);
            vi[e] = fmaf(2.f, vi[e], -1.f);
        }
        xr[e] = vi[e] - v0[e];
        xt[e] = fmaf(bc, z[e], fmaf(ac, xr[e], v0[e]));
    }
    store4<VEC>(a.x_in + (int64_t)b * 2 * npix + i0, n, xt);
    store4<VEC>(a.x_in + ((int64_t)b * 2 + 1) * npix + i0, n, vi);
    store4<VEC>(a.x_res + row, n, xr);
    if (MODE == MODE_KEYED) store4<VEC>(a.noise_out + row, n, z);
    if (a.x0) store4<VEC>(a.x0 + row, n, v0);
}

}  // namespace
