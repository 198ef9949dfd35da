// fd_obj_pixel.h -- one pixel of a sampler step for every objective of model_predictions and the two-U-Net model
// (src/DADiff.py:1168-1207 + 1142-1151, 1226-1229, 1317-1318, 1344), shared by the step kernels that must agree bit for bit:
// fd_sched.hip (fd_res_step_obj_keyed, one slice = one row) and fd_tiles_step.hip (the same update on tile rows whose model outputs
// are blended across tiles first).  The fused multiply-adds are written out and the compiler forms none of its own, so a caller's
// 16-byte and one-pixel forms round alike.  The products and differences are contracted the way the compiler contracts
// fd_small.hip's res_step_obj_kernel (x - a y - b n = fma(-b, n, fma(-a, y, x)), x - k pr = fma(-k, pr, x), c1 x + c2 pr + c3 xs =
// fma(c3, xs, fma(c2, pr, c1 x))): that kernel keeps its own runtime-`mode` text, and these have its bits.
#pragma once
#include "fd_common.h"

namespace {

struct obj_row { float a, bb, oma, c1, c2, c3, sd; };

// the predictions of `MODE`: pred_res and x_start from the raw outputs o0 / o1, the state x and the input xi
template <int MODE>
__device__ __forceinline__ void obj_predict(float a, float bb, float oma, float o0, float o1, float x, float xi, float &pr, float &xs) {
#pragma clang fp contract(off)
    if (MODE == 0) {
        pr = fd_clamp1(o0);
        xs = fd_clamp1(xi - pr);
    } else if (MODE == 1) {
        xs = fd_clamp1(fmaf(-bb, o1, fmaf(-a, xi, x)) / oma);
        pr = fd_clamp1(xi - xs);
    } else if (MODE == 2) {
        pr = fd_clamp1(o0);
        xs = fd_clamp1(fmaf(-bb, o1, fmaf(-a, pr, x)));
    } else {
        pr = fd_clamp1(xi - o0);
        xs = fd_clamp1(o0);
    }
}

// the ancestral step (res_step_obj_kernel's step == 2): the posterior mean of row r plus sd z
template <int MODE>
__device__ __forceinline__ float obj_pixel(const obj_row &r, float o0, float o1, float x, float xi, float z) {
#pragma clang fp contract(off)
    float pr, xs;
    obj_predict<MODE>(r.a, r.bb, r.oma, o0, o1, x, xi, pr, xs);
    return fmaf(r.sd, z, fmaf(r.c3, xs, fmaf(r.c2, pr, r.c1 * x)));
}

// the DDIM step without noise (res_step_obj_kernel's step == 1): x_start on the last step, x - alpha pred_res before it
template <int MODE>
__device__ __forceinline__ float obj_ddim_pixel(float a, float bb, float oma, float alpha, bool last, float o0, float o1, float x,
                                                float xi) {
#pragma clang fp contract(off)
    float pr, xs;
    obj_predict<MODE>(a, bb, oma, o0, o1, x, xi, pr, xs);
    return last ? xs : fmaf(-alpha, pr, x);
}

}  // namespace
