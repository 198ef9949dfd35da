// fd_grad_sum.hip -- the gradient sum of data-parallel training (diffusion_train.GradReducer), over the optimiser's chunk table and
// per-tensor pointer table (fd_train_step.hip) and one flat fp32 buffer per rank:
//
//   fd_grads_pack_f32      flat[offs[i] + k] = g_i[k] for every tensor with a gradient (zeros for one without, zeros in the padding),
//                          the tail's floats behind them; with `zero`, g = 0 afterwards (the next backward starts from 0)
//   fd_grads_rank_sum_f32  v = first ? 0 : acc[i]; v = v + recv[r][i] for r = 0 .. W - 1, strictly in that order; if `last` v goes to
//                          the gradients through the tables, otherwise to acc.  The tail always goes to acc.
//
// The flat layout is the one of the optimiser's moments: tensor i starts at offs[i], a multiple of 4, offs[i + 1] - offs[i] = numel_i
// rounded up to 4; P is their total and the tail is the TAIL floats behind it.  Bandwidth kernels: a lane owns 4 consecutive floats,
// the flat side is always one 16-byte access, the gradient side is one where the table's alignment flag allows it and scalar with the
// same element ownership otherwise, so both paths give the same bits.  Plain adds in a fixed order: no fmaf, no atomics, nothing that
// depends on W but the number of terms.  The same code in both builds of the library.
#include "fd_train_common.h"

namespace {

constexpr int GS_CHUNK = 4096;         // fd_opt_chunk_elems(): 256 lanes x 4 vectors of 4
constexpr int GS_VPL = GS_CHUNK / 1024;
constexpr int GS_TT_COLS = 8;          // per-tensor table row: p, g, m, v, ema, flags, 0, 0
constexpr int64_t GS_ACTIVE = 1, GS_VEC = 2;
constexpr int GS_TAIL = 4;             // floats behind the gradients (the losses of the micro-batch, one per U-Net)
constexpr int GS_ROWS = 8;             // rows of recv in flight per lane before the first add of a batch
constexpr int GS_MAX_W = 64;

struct GsChunk {
    float *g;
    int64_t flat;                      // where the chunk starts in a flat buffer
    int len;
    bool active, vec;
};

__device__ __forceinline__ GsChunk gs_chunk(const int64_t *__restrict__ chunks, const int64_t *__restrict__ tensors,
                                            const int64_t *__restrict__ offs) {
    const int64_t *c = chunks + 3 * (int64_t)blockIdx.x;
    const int64_t *row = tensors + GS_TT_COLS * c[0];
    GsChunk o;
    o.active = (row[5] & GS_ACTIVE) != 0;
    o.vec = (row[5] & GS_VEC) != 0;
    o.g = o.active ? (float *)row[1] + c[1] : nullptr;
    o.flat = offs[c[0]] + c[1];
    o.len = (int)c[2];
    return o;
}

// grid (nchunk + 1): one workgroup per chunk, the last one writes the tail
__global__ __launch_bounds__(256) void grads_pack_kernel(const int64_t *__restrict__ chunks, const int64_t *__restrict__ tensors,
                                                        const int64_t *__restrict__ offs, int nchunk, float *__restrict__ flat,
                                                        int64_t P, const float *__restrict__ tail, int ntail, int zero) {
    const int tid = threadIdx.x;
    if ((int)blockIdx.x == nchunk) {
        if (tid < GS_TAIL) flat[P + tid] = tid < ntail ? tail[tid] : 0.f;
        return;
    }
    const GsChunk o = gs_chunk(chunks, tensors, offs);
    const float zeros[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < GS_VPL; ++j) {
        const int i0 = 4 * (j * 256 + tid);
        if (i0 >= o.len) continue;
        const int n = min(4, o.len - i0);
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (o.active) {
            if (o.vec && n == 4) load4<true>(o.g + i0, 4, v);
            else load4<false>(o.g + i0, n, v);                           // the padding reads as 0
        }
        store4<true>(flat + o.flat + i0, 4, v);                          // a tensor's flat range is padded to 4: always whole
        if (zero && o.active) {
            if (o.vec && n == 4) store4<true>(o.g + i0, 4, zeros);
            else store4<false>(o.g + i0, n, zeros);
        }
    }
}

// v += recv[r][i .. i + 4) for r = 0 .. W - 1 in order; the loads of up to GS_ROWS rows are issued before the first add of the batch
__device__ __forceinline__ void rank_sum4(const float *__restrict__ recv, int W, int64_t N, int64_t i, float v[4]) {
    for (int r0 = 0; r0 < W; r0 += GS_ROWS) {
        f32x4 q[GS_ROWS];
#pragma unroll
        for (int k = 0; k < GS_ROWS; ++k)
            if (r0 + k < W) q[k] = *(const f32x4 *)(recv + (int64_t)(r0 + k) * N + i);
#pragma unroll
        for (int k = 0; k < GS_ROWS; ++k)
            if (r0 + k < W) {
                v[0] = v[0] + q[k].x;
                v[1] = v[1] + q[k].y;
                v[2] = v[2] + q[k].z;
                v[3] = v[3] + q[k].w;
            }
    }
}

// grid (nchunk + 1): one workgroup per chunk, the last one sums the tail (always into acc)
__global__ __launch_bounds__(256) void grads_rank_sum_kernel(const int64_t *__restrict__ chunks, const int64_t *__restrict__ tensors,
                                                            const int64_t *__restrict__ offs, int nchunk,
                                                            const float *__restrict__ recv, int W, int64_t N, float *__restrict__ acc,
                                                            int64_t P, int first, int last) {
    const int tid = threadIdx.x;
    if ((int)blockIdx.x == nchunk) {
        if (tid == 0) {
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (!first) load4<true>(acc + P, 4, v);
            rank_sum4(recv, W, N, P, v);
            store4<true>(acc + P, 4, v);
        }
        return;
    }
    const GsChunk o = gs_chunk(chunks, tensors, offs);
    if (last && !o.active) return;                                       // a tensor without a gradient is not touched
#pragma unroll
    for (int j = 0; j < GS_VPL; ++j) {
        const int i0 = 4 * (j * 256 + tid);
        if (i0 >= o.len) continue;
        const int n = min(4, o.len - i0);
        const int64_t i = o.flat + i0;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (!first) load4<true>(acc + i, 4, v);
        rank_sum4(recv, W, N, i, v);
        if (!last) store4<true>(acc + i, 4, v);
        else if (o.vec && n == 4) store4<true>(o.g + i0, 4, v);
        else store4<false>(o.g + i0, n, v);
    }
}

}  // namespace

extern "C" int fd_grads_tail_floats(void) { return GS_TAIL; }

extern "C" int fd_grads_pack_f32(const int64_t *chunks, const int64_t *tensors, const int64_t *offs, int nchunk, float *flat,
                                 int64_t P, const float *tail, int ntail, int zero, void *stream) {
    FD_REQUIRE(chunks && tensors && offs && flat, "fd_grads_pack_f32: null pointer");
    FD_REQUIRE(nchunk > 0 && P > 0 && P % 4 == 0, "fd_grads_pack_f32: unsupported sizes nchunk=%d P=%lld (P a positive multiple of 4)",
               nchunk, (long long)P);
    FD_REQUIRE(ntail >= 0 && ntail <= GS_TAIL && (ntail == 0 || tail), "fd_grads_pack_f32: the tail holds at most %d floats (got %d)",
               GS_TAIL, ntail);
    FD_REQUIRE(al16(flat), "fd_grads_pack_f32: flat must be 16-byte aligned");
    FD_REQUIRE(fd_opt_chunk_elems() == GS_CHUNK, "fd_grads_pack_f32: the chunk table is cut in %d elements, this file expects %d",
               fd_opt_chunk_elems(), GS_CHUNK);
    hipLaunchKernelGGL(grads_pack_kernel, dim3((unsigned)nchunk + 1), dim3(256), 0, (hipStream_t)stream, chunks, tensors, offs, nchunk,
                       flat, P, tail, ntail, zero);
    FD_LAUNCH_OK("fd_grads_pack_f32");
    return FD_OK;
}

extern "C" int fd_grads_rank_sum_f32(const int64_t *chunks, const int64_t *tensors, const int64_t *offs, int nchunk, const float *recv,
                                     int W, int64_t N, float *acc, int64_t P, int first, int last, void *stream) {
    FD_REQUIRE(chunks && tensors && offs && recv && acc, "fd_grads_rank_sum_f32: null pointer");
    FD_REQUIRE(nchunk > 0 && P > 0 && P % 4 == 0 && N == P + GS_TAIL,
               "fd_grads_rank_sum_f32: unsupported sizes nchunk=%d P=%lld N=%lld (P a positive multiple of 4, N = P + %d)", nchunk,
               (long long)P, (long long)N, GS_TAIL);
    FD_REQUIRE(W >= 1 && W <= GS_MAX_W, "fd_grads_rank_sum_f32: W must be in [1, %d] (got %d)", GS_MAX_W, W);
    FD_REQUIRE(al16(recv) && al16(acc), "fd_grads_rank_sum_f32: recv and acc must be 16-byte aligned");
    FD_REQUIRE(fd_opt_chunk_elems() == GS_CHUNK, "fd_grads_rank_sum_f32: the chunk table is cut in %d elements, this file expects %d",
               fd_opt_chunk_elems(), GS_CHUNK);
    hipLaunchKernelGGL(grads_rank_sum_kernel, dim3((unsigned)nchunk + 1), dim3(256), 0, (hipStream_t)stream, chunks, tensors, offs,
                       nchunk, recv, W, N, acc, P, first, last);
    FD_LAUNCH_OK("fd_grads_rank_sum_f32");
    return FD_OK;
}
