/* founddiff_hip.h -- C ABI of libfounddiff_hip.so (MI355X / gfx950 only).
 *
 * The reference (hao1635/FoundDiff) is pure PyTorch with exactly ONE native boundary on the
 * sampling path:  selective_scan_cuda_core.fwd(u, delta, A, B, C, D, delta_bias,
 * delta_softplus, nrows)  at /root/reference/src/emamba2.py:154 (third-party CUDA, not
 * vendored).  Everything else bottoms out in ATen.  This library replaces that op AND the
 * ATen calls of the per-timestep denoiser with hand-written HIP kernels; each entry point
 * below cites the reference lines it replaces.
 *
 * Conventions
 *   - plain C: raw DEVICE pointers, ints, a hipStream_t passed as void*; no torch types.
 *   - activations are NHWC (channels-last) `dtype` elements: FD_F32 (parity mode, fp32
 *     storage + exact-f32 MFMA) or FD_BF16 (bf16 storage, bf16 MFMA, fp32 accumulate).
 *     Statistics, scan state, gates, biases and all "small" vectors are always fp32.
 *   - the caller owns every buffer incl. workspaces; the library allocates nothing, keeps
 *     no state, never synchronises: work is enqueued on `stream` (graph-capturable).
 *   - return 0 on success, <0 on error (fd_last_error() gives the text, thread-local).
 */
#ifndef FOUNDDIFF_HIP_H
#define FOUNDDIFF_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FD_F32 0
#define FD_BF16 1

#define FD_OK 0
#define FD_ERR_ARG (-1)
#define FD_ERR_LAUNCH (-2)

int fd_version(void);
/* Development switches (round 6).  The release build (what founddiff_amd.build.build() ships: -DFD_RELEASE) reads NO environment
 * variable: every tuning switch of the dispatch code is compiled to its default.  A development build (FOUNDDIFF_DEV_BUILD=1)
 * reads the FD_* variables of founddiff_amd/csrc/fd_common.h (FD_DEV_SWITCHES) once, on the first call that needs one.  Returns a
 * static string: "release build: ..." or the switches that are set.                                                    */
const char *fd_dev_options(void);
/* The 16-bit type behind dtype code FD_BF16 in THIS build of the library: 0 = bfloat16 (libfounddiff_hip.so, the default), 1 = IEEE
 * binary16 (libfounddiff_hip_f16.so: the same sources compiled with -DFD_HALF_F16; founddiff_amd's precision='fp16').  Every entry
 * point below that says "bf16" then reads and writes binary16 instead; fp32 arguments are unchanged.  The fp32-storage split mode
 * (FD_OPT_F32_SPLIT) and the fp8 weights mode are meant for the default build only.                                       */
int fd_half_format(void);
const char *fd_last_error(void);

/* ---- implicit-GEMM convolution / GEMM on MFMA -------------------------------------------
 * Replaces F.conv2d / nn.Linear / torch.cat / nn.Upsample(nearest) on the denoiser path:
 *   3x3 WS-conv of Block          src/DADiff.py:145-154, 221   (weights standardised at pack time)
 *   4x4-s2 Downsample, Upsample   src/DADiff.py:128-136
 *   7x7 init_conv, 1x1 res_conv   src/DADiff.py:558, 407-408, 430
 *   skip concat                   src/DADiff.py:727, 733       (two-source A operand)
 *   in_proj / out_proj / x_proj   src/emamba2.py:717, 748, 335 (x_proj = 4 stride-2 1x1 convs)
 *   qkv / project_out             src/DADiff.py:266, 283
 *   RN50 convs of DA-CLIP         src/DACLIP.py:198-211, 329-349 (BN folded at pack time)
 * out[b,oh,ow,n] = epi( bias[n] + sum_{kh,kw,c} in[b, (oh*s-ph+kh)(>>1 if upsample), ..., c] * w[n,kh,kw,c] )
 */
#define FD_EPI_NONE 0       /* acc + bias                                                      */
#define FD_EPI_SILU_SPLIT 1 /* SiLU on output channels >= epi_split (in_proj's z half)        */
#define FD_EPI_RELU 2
#define FD_EPI_GATE_RES 3   /* res[m,n] + gate[b,n] * (acc + bias)   adaLN-gated residual     */
#define FD_EPI_RES_RELU 4   /* relu(acc + bias + res[m,n])           RN50 bottleneck tail     */
#define FD_EPI_GNSILU_ADD 5 /* acc + bias + silu(GN(h[m,n]))         res_conv + Block output  */
/* GNSILU_ADD, then the denoiser's last 1x1 (final_conv, Cout -> 1) and the sampler's update in the same pass: the
 * block's Cout-channel output is never written.  o = fin_b + sum_n fin_w[n] * value[m,n] -> fin_out[b][m] (fp32);
 * fin_mode 1: + the DDIM update of src/DADiff.py:1203-1206, 1317-1318, 1344 on the fp32 image planes:
 *   pr = clamp(o, +-1);  fin_img[b][m] <- fin_last ? clamp(fin_xin - pr, +-1) : fin_img - fin_alpha * pr.
 * Streaming row-GEMM only (bf16, fd_conv_prologue_ok).                                              */
#define FD_EPI_GNSILU_ADD_FINAL 6

typedef struct fd_conv_params {
    int32_t dtype;              /* FD_F32 | FD_BF16: type of in0/in1/weight/res/h            */
    int32_t out_f32;            /* 1: `out` is fp32 regardless of dtype                       */
    const void *in0;            /* first source  [B,H,W,ld0], channels [off0, off0+c0)        */
    const void *in1;            /* optional second source (channel concat after in0) or NULL  */
    int32_t c0, ld0, off0;
    int32_t c1, ld1, off1;
    int32_t B, H, W;            /* source spatial size (before the optional x2 upsample)      */
    int32_t upsample;           /* 1: nearest x2 before the conv                              */
    int32_t KH, KW, stride, pad_h, pad_w;   /* pads may be negative (sub-grid origin)         */
    int32_t OH, OW;
    int32_t ndir;               /* 1, or 4: SS2D directions; dir k uses pad=(-(k&1), -(k>>1)),
                                   weight + k*w_dir_stride, out + k*out_dir_stride            */
    const void *weight;         /* [Cout][KH*KW*(c0+c1)], K order (kh,kw,c)                   */
    int64_t w_batch_stride;     /* elements between per-batch weight sets (0: shared)         */
    int64_t w_dir_stride;
    const float *bias;          /* [Cout] or NULL                                             */
    int32_t Cout;
    void *out;                  /* [B,OH,OW,ldo] channels [offo, offo+Cout)                   */
    int32_t ldo, offo;
    int64_t out_dir_stride;     /* elements                                                   */
    int32_t epilogue;
    int32_t epi_split;
    const void *res;            /* GATE_RES / RES_RELU: [B,OH,OW,ld_res] (dtype)              */
    int32_t ld_res, off_res;
    const float *gate;          /* GATE_RES: [B][gate_ld] fp32, entries gate[b*gate_ld + n]   */
    int32_t gate_ld;
    const void *h;              /* GNSILU_ADD: raw conv output [B,OH,OW,Cout] (dtype)          */
    const float *gn_mean_rstd;  /* GNSILU_ADD: [B][G][2]                                      */
    const float *gn_gamma, *gn_beta;
    int32_t gn_groups;
    float *stats_partial;       /* optional: per-(b, m-tile, channel) sum & sumsq of the
                                   stored values, [B][mtiles][Cout][2]; see fd_conv_mtiles    */
    /* LayerNorm over the Cin channels of in0 fused into the operand load.  Only the bf16
     * streaming row-GEMM path implements it: ask fd_conv_prologue_ok() first.
     *   LN_MOD : x' = LN(x)*(1+scale[b]) + shift[b]           src/DADiff.py:450-451,486-487
     *   LN_GATE: x' = LN(x)*z[m] + local[b]  (shift = local)  src/emamba2.py:365,747-748     */
    int32_t prologue;
    float ln_eps;
    const float *ln_gamma, *ln_beta;   /* [Cin] or NULL (LN_MOD without affine)              */
    const float *ln_shift, *ln_scale;  /* entries [b*ln_ld + c]                               */
    int32_t ln_ld;
    const void *ln_z;                  /* LN_GATE: [B,H,W,ln_ldz], channels [ln_offz, +Cin)   */
    int32_t ln_ldz, ln_offz;
    /* fp8 weights (BASELINE configs[4]): the same [Cout][KH*KW*Cin] matrix as OCP e4m3 bytes,
     * w_f8[n][k] = e4m3(weight[n][k] / w_scale[n]), one fp32 scale per output channel.  Used by the
     * 3x3 halo kernel where the K axis splits into 128-channel slabs (fd_conv_fp8_ok): the bf16 halo is
     * converted to e4m3 (x act_scale, a power of two) once per slab on its way into LDS and the product
     * runs on v_mfma_scale_f32_16x16x128_f8f6f4 (2x the bf16 rate), fp32 accumulation;
     * out = acc * w_scale[n] / act_scale + bias.  NULL: bf16 weights.  Other convs ignore these.       */
    const void *weight_f8;
    const float *w_scale;
    float act_scale;
    /* fp32 storage only: 1 = split-bf16 contraction (x = hi + lo in bf16, hi.hi + hi.lo + lo.hi on the bf16 MFMA,
     * fp32 accumulation: ~2^-16 per product) instead of the exact-f32 MFMA.  The parity mode leaves it 0.       */
    int32_t f32_split;
    /* FD_EPI_GNSILU_ADD_FINAL                                                                                  */
    const float *fin_w;                /* [Cout]                                              */
    float fin_b;
    float *fin_out;                    /* [B][H*W] fp32 model output                          */
    int32_t fin_mode, fin_last;        /* 0: fin_out only; 1: + DDIM update of fin_img        */
    float *fin_img;                    /* [B][H*W] fp32 x_t, updated in place                 */
    const float *fin_xin;              /* [B][H*W] fp32 x_input                               */
    float fin_alpha;
    /* FD_PRO_LN_GATE_ZRE (round 4): LN_GATE whose z operand is RECOMPUTED from the block input instead of read:
     *   z[m] = SiLU(zre_w . (LN(res[m]) * gamma (1 + scale[b]) + beta (1 + scale[b]) + shift[b]))
     * i.e. the z half of SS2D's in_proj (src/emamba2.py:716-719) applied to the adaLN-modulated norm1 of the Mamba
     * block's input (src/DADiff.py:450-451, 477-481), which out_proj reads anyway as its residual (`res`, GATE_RES).
     * z then never exists in HBM.  Needs Cin == 2 * Cout (d_inner = 2 * dim); ask fd_conv_prologue_ok().          */
    const void *zre_w;                 /* [Cin][Cout] (dtype): rows d_inner .. 2 d_inner - 1 of in_proj.weight    */
    const float *zre_gamma, *zre_beta; /* [Cout] norm1 affine or NULL                                             */
    const float *zre_shift, *zre_scale;/* entries [b*zre_ld + c]                                                  */
    int32_t zre_ld;
    float zre_eps;
    /* Up-sampling 3x3 convolutions (`upsample` = 1, KH = KW = 3: nn.Upsample(scale_factor=2, nearest) -> Conv2d,
     * src/DADiff.py:121-127) as four 2x2 convolutions on the source grid, one per output parity class (round 5, bf16 halo
     * kernel): weight_up2x[n][cls][r][c][ci], cls = 2 a + b for output pixel (2 i + a, 2 j + b), tap (r, c) reads source pixel
     * (i + a + r - 1, j + b + c - 1) with the weights of the 3x3 taps that fall on that pixel summed (a = 0: r = 0 <- kh 0,
     * r = 1 <- kh 1 + 2; a = 1: r = 0 <- kh 0 + 1, r = 1 <- kh 2; columns likewise), i.e. [Cout][16 * Cin] in dtype.  The same
     * convolution in exact arithmetic with 4 instead of 9 MACs per output.  NULL: the 9-tap form.  Other convs ignore it.
     * `upsample` = 2 (otherwise the same as 1) asks for one workgroup per (tile, parity class) instead of per tile: four times
     * the workgroups for a batch that does not fill the chip; the results are the same bits.                                 */
    const void *weight_up2x;
    /* fp32 storage with f32_split = 1, 3x3 / stride 1 / pad 1 (round 5): the weight matrix pre-split into its bf16 halves,
     * w = hi + lo with hi = bf16(w), lo = bf16(w - hi), each [Cout][9 * Cin] bf16.  With both set the convolution runs on the
     * halo-tiled kernel (three bf16 MFMA units per 64-channel slab: x_hi.w_hi + x_hi.w_lo + x_lo.w_hi) instead of the generic
     * split implicit GEMM; `weight` (fp32) stays the reference copy.  NULL: the generic form.                              */
    const void *weight_split_hi, *weight_split_lo;
    /* Both of the above at once (fp32 storage, f32_split = 1, `upsample` != 0, 3x3): the sub-pixel matrix of weight_up2x, built
     * from the fp32 weights and pre-split into bf16 halves, [Cout][16 * Cin] each: four 2x2 split-bf16 convolutions on the
     * source grid.  NULL: the 9-tap split form through the up-sampling index map.                                        */
    const void *weight_up2x_split_hi, *weight_up2x_split_lo;
} fd_conv_params;

/* 1 if fd_conv2d would run `p` (weight_f8 / w_scale set) on the fp8 MFMA path.                        */
int fd_conv_fp8_ok(const fd_conv_params *p);

#define FD_PRO_NONE 0
#define FD_PRO_LN_MOD 1
#define FD_PRO_LN_GATE 2
#define FD_PRO_LN_GATE_ZRE 3
/* 1 if this conv runs on the streaming row-GEMM kernel (1x1, bf16, Cin <= 256, >= 16384 pixels
 * per image, weights fit LDS) and may therefore carry a fused LN prologue.                    */
int fd_conv_prologue_ok(const fd_conv_params *p);

int fd_conv_mtiles(int OH, int OW);         /* number of m-tiles per image (for workspaces)  */
/* kernel fd_conv2d will run for p: 10 row-GEMM, 11 halo 3x3 (12: its fp8 form), 0..6 implicit-GEMM <BM,BN> =
 * <128,128>, <128,64>, <64,128>, <64,64>, <128,256>, <256,256>, <128,32> (profiling / roofline
 * bookkeeping; ids 4 and 5 depend on the batch size but give bitwise identical outputs)      */
int fd_conv_kernel_id(const fd_conv_params *p);
/* fd_conv_kernel_id(p) | pw << 8: pw = 1 when an implicit-GEMM tile (ids 0..6) runs with the bf16 pointwise loader (1x1, stride 1,
 * Cin and c0 multiples of 64, 8-channel-aligned output, no GroupNorm sums) instead of the general gather.  Host only.       */
int fd_conv_form(const fd_conv_params *p);
/* The launch plan of the streaming row-GEMM (fd_conv_kernel_id 10 and 17) for p.  Host only: touches no device.  Returns 1 and fills
 * form[0 .. 9] when p runs there (fd_conv_prologue_ok), 0 (form untouched) otherwise.  Field order:
 *   [0] kernel id: 10 = 16-bit storage, 17 = fp32 storage with split-bf16 contractions
 *   [1] KS = Cin / 32   [2] PRO = p.prologue (3: a z-recompute kernel, see [9])   [3] EPI = p.epilogue
 *   [4] NT: threads per workgroup, 256 / 512 / 768 from the LDS bytes of the weight image and the register budget of (KS, PRO)
 *   [5] S: 16-pixel subtiles per wave iteration (2 for Cin <= 64 in 16-bit storage, else 1)
 *   [6] wtiles = ceil(H * W / (16 S)): wave tiles per image   [7] grid x (grid y = B); wave w of workgroup x walks the tiles
 *       x * NT/64 + w, + grid x * NT/64, ...   [8] dynamic LDS bytes
 *   [9] z-recompute kernel: 0 none, 1 = 16-bit Cin 128, 2 = 16-bit Cin 256, 3 = fp32 storage Cin 128
 * fd_conv2d launches exactly this plan, and fails (rather than launch nothing) if no kernel was compiled for it.
 * FD_EPI_GNSILU_ADD_FINAL stores nothing through p.out: the block output exists only inside the fin_w dot product.            */
int fd_gemm_rows_form(const fd_conv_params *p, int *form);
int fd_conv2d(const fd_conv_params *p, void *stream);

/* GroupNorm statistics from the conv's partial sums -> mean_rstd [B][G][2] (nn.GroupNorm,
 * src/DADiff.py:217,222).  */
int fd_gn_finalize(const float *stats_partial, int B, int mtiles, int C, int groups, int64_t hw,
                   float eps, float *mean_rstd, void *stream);
/* out = silu(GN(h)) (+ res)  -- Block tail + identity residual, src/DADiff.py:222-228, 430. */
int fd_gn_silu_apply(int dtype, const void *h, const float *mean_rstd, const float *gamma,
                     const float *beta, const void *res, void *out, int B, int64_t hw, int C,
                     int groups, void *stream);
/* The tail of an identity-residual ResnetBlock AND the down-sampling convolution behind it in one pass (round 4, bf16, C = 64):
 *   skip = x + SiLU(GroupNorm(h)) -- bit for bit fd_gn_silu_apply's result -- and
 *   out  = Conv2d(C, Cout, 4, stride 2, padding 1)(skip) + bias        (src/DADiff.py:128-131, 213-229, 418-430, 578-584)
 * h, x, skip [B,H,W,64]; mean_rstd [B][groups][2] from fd_gn_finalize; w [Cout][16 taps x 64] in K order (kh, kw, c) as for
 * fd_conv2d; out [B,H/2,W/2,Cout], Cout in {64, 128}; H % 16 == 0, W % 32 == 0.  The applied tensor is read back by nothing:
 * the convolution runs on the tile the apply left in LDS, with the weights resident in registers.                       */
int fd_gn_apply_down4x4_ok(int dtype_opts, int C, int Cout, int H, int W);
int fd_gn_apply_down4x4(int dtype, const void *h, const void *x, const float *mean_rstd, const float *gamma,
                        const float *beta, int groups, void *skip, const void *w, const float *bias, void *out,
                        int B, int H, int W, int C, int Cout, void *stream);

/* ---- LayerNorm family (channel-last rows) ------------------------------------------------
 * fd_ln_modulate: out = LN(x) * (1 + scale[b]) + shift[b]      src/DADiff.py:450-451, 486-487
 *   gamma/beta may be NULL (norm2: elementwise_affine=False).  */
int fd_ln_modulate(int dtype, const void *x, const float *gamma, const float *beta, float eps,
                   const float *shift, const float *scale, int mod_ld, void *out, int B,
                   int64_t hw, int C, void *stream);
/* fd_ln_gate: out = LN(y) * z + local[b]   (out_norm, y*z, +local)  src/emamba2.py:365, 747-748
 *   z has pixel stride ldz and channel offset offz (the z half of in_proj's output).         */
int fd_ln_gate(int dtype, const void *y, const float *gamma, const float *beta, float eps,
               const void *z, int ldz, int offz, const float *local, int local_ld, void *out,
               int B, int64_t hw, int C, void *stream);

/* ---- depthwise 3x3 conv, NHWC (SS2D conv2d + SiLU, qkv_dwconv)  src/emamba2.py:722,
 *      src/DADiff.py:266.  weight [9][C] fp32 (tap-major), bias [C] or NULL.                 */
int fd_dwconv3x3(int dtype, const void *in, int ld_in, int off_in, const float *weight,
                 const float *bias, int silu, void *out, int ld_out, int off_out, int B, int H,
                 int W, int C, void *stream);

/* ---- fused LayerNorm+modulate -> 1x1 conv -> depthwise 3x3 (bf16, Cin = 64, >= 32768 px/image)
 * Replaces, in one pass over the pixels, the pairs
 *   SS2D   in_proj + conv2d(3x3, groups=D)+SiLU (x half), SiLU (z half)   src/emamba2.py:716-722
 *   attn   qkv + qkv_dwconv                                               src/DADiff.py:266, 275
 * including the adaLN-modulated LayerNorm in front of them (src/DADiff.py:480-487).
 *   x      [B,H,W,ld_x] channels [off_x, +Cin)
 *   w_pw   bf16 [Cdw + Cz][Cin]: rows [0, Cdw) feed the depthwise conv, rows [Cdw, Cdw+Cz) are passed
 *          through SiLU to out_z (Cz = 0: none)
 *   w_dw   [9][Cdw/2] 32-bit words of fp16 tap weights, tap = 3*dy + dx, word j = (channel 2j low, 2j+1 high): the
 *          depthwise runs on v_pk_fma_f16 (the 1x1 output is kept in LDS as fp16 channel pairs, the 9-tap sum is
 *          accumulated in fp16 starting from the bias rounded to fp16 (toward zero); SiLU in fp32).  b_dw [Cdw] fp32 or NULL
 *   ln_*   as fd_conv_params' LN_MOD prologue (gamma/beta may be NULL)
 * fd_pw_dw3x3_ok: 1 if the shape is served (callers fall back to fd_conv2d + fd_dwconv3x3); `dtype | FD_OPT_LOW_LATENCY`
 *   answers for the one-slice kernel set (Cin = 128 stays unfused there).   */
int fd_pw_dw3x3_ok(int dtype, int Cin, int Cdw, int Cz, int H, int W);
int fd_pw_dw3x3(int dtype, const void *x, int ld_x, int off_x, int Cin, const float *ln_gamma,
                const float *ln_beta, float ln_eps, const float *ln_shift, const float *ln_scale,
                int ln_ld, const void *w_pw, int Cdw, const uint32_t *w_dw, const float *b_dw,
                int dw_silu, void *out_dw, int ld_dw, int off_dw, int Cz, void *out_z, int ld_z,
                int off_z, int B, int H, int W, void *stream);

/* ---- the qkv form of the above with the channel attention's statistics folded in (src/DADiff.py:266-276):
 * qkv (C -> 3C) -> qkv_dwconv -> per head L2 norms of q, k over all pixels and the 32x32 Gram q k^T.  q and k never
 * reach HBM: only v (out_v, [B,H,W,ld_v] channels [off_v, +64)) and one partial per workgroup do --
 * partial [B][2 heads][nblk][1024 + 64] fp32 in fd_chan_attn_gram's layout (Gram rows = q channels; then sum q^2,
 * sum k^2), nblk = fd_pw_dw3x3_gram_nblk(H, W), reduced in fixed order by fd_chan_attn_weff.  bf16, Cin = 64 (two
 * heads), w_pw [192][64] (q | k | v rows), w_dw [9][96] as for fd_pw_dw3x3, no bias; q and k are fp16 on chip (f16 MFMA):
 * their magnitudes must sit inside fp16's range -- they are L2-normalised per channel afterwards, so a per-channel
 * power-of-two scale folded into their w_pw rows / w_dw taps is free (founddiff_amd/engine.py does that at pack time). */
int fd_pw_dw3x3_gram_ok(int dtype, int Cin, int H, int W);
int fd_pw_dw3x3_gram_nblk(int H, int W);
/* ... with `dtype | FD_OPT_LOW_LATENCY` passed to fd_pw_dw3x3_gram (4 instead of 8 tiles per workgroup: the kernel set for ONE
 * slice, as for the scan) the partial count is fd_pw_dw3x3_gram_nblk_opts(dtype_opts, H, W).                         */
int fd_pw_dw3x3_gram_nblk_opts(int dtype_opts, int H, int W);
int fd_pw_dw3x3_gram(int dtype, const void *x, int ld_x, int off_x, int Cin, const float *ln_gamma,
                     const float *ln_beta, float ln_eps, const float *ln_shift, const float *ln_scale,
                     int ln_ld, const void *w_pw, const uint32_t *w_dw, void *out_v, int ld_v, int off_v,
                     float *partial, int B, int H, int W, void *stream);
/* out_v may be NULL (round 4): q and k only, for use with fd_pw_dw3x3_proj below, which recomputes v where it is
 * consumed.
 *
 * The v branch of the same attention through project_out and the block's gated residual (src/DADiff.py:266-285, 483-488):
 *   out = x + gate[b] . (w2[b] . dwconv3x3(w_pw . (LN(x) (1 + scale[b]) + shift[b])))
 * w_pw [64][64] (the v rows of qkv.weight), w_dw [9][32] fp16 channel pairs (the v taps of qkv_dwconv, fd_pw_dw3x3's
 * layout), w2 [B][64][64] = fd_chan_attn_weff's output, gate entries [b*gate_ld + n].  bf16, Cin = 64; v never reaches
 * HBM.  The depthwise output is rounded to bf16 before the second 1x1, as the stored v of the unfused sequence is.   */
int fd_pw_dw3x3_proj_ok(int dtype_opts, int Cin, int H, int W);
int fd_pw_dw3x3_proj(int dtype, const void *x, int ld_x, int off_x, int Cin, const float *ln_gamma,
                     const float *ln_beta, float ln_eps, const float *ln_shift, const float *ln_scale,
                     int ln_ld, const void *w_pw, const uint32_t *w_dw, const void *w2, const float *gate,
                     int gate_ld, void *out, int ld_o, int off_o, int B, int H, int W, void *stream);

/* ---- the three fused kernels above on FP32 STORAGE with split-bf16 contractions (round 6, fd_pwdw32.hip): the 64-channel
 * Mamba blocks of the `fp32s` engine (fp32 activations, every dense product as three bf16 MFMAs on hi / lo operand halves,
 * fp32 LayerNorm / depthwise / accumulation; the exact-f32 MFMA for the Gram).  Weights come as the checkpoint's fp32 values:
 *   w_pw_hi / w_pw_lo  bf16 [rows][64]: the checkpoint's fp32 1x1 weights split by the caller, hi = bf16(w), lo = bf16(w - hi);
 *   w_dw fp32 [9][ld_wdw] tap-major, column = w_pw row; b_dw fp32 [rows] or NULL
 * Same reference lines as the bf16 forms: src/emamba2.py:716-722 (in_proj x half + conv2d + SiLU; Cdw rows, z is recomputed by
 * fd_conv2d's FD_PRO_LN_GATE_ZRE), src/DADiff.py:266-276 (q, k rows 0..127 of qkv.weight -> qkv_dwconv -> per-head Gram and L2
 * norms; partial [B][2][nblk][1024 + 64] in fd_chan_attn_gram's layout, nblk = fd_pw_dw3x3_gram_f32_nblk(H, W)),
 * src/DADiff.py:266-285, 483-488 (v rows -> qkv_dwconv -> w2[b] = fd_chan_attn_weff's fp32 output -> x + gate . ()).
 * Cin = 64, H % 8 == 0, W % 16 == 0 (W % 8 for the Gram / project_out forms), >= 16384 px per image.               */
int fd_pw_dw3x3_f32_ok(int dtype, int Cin, int Cdw, int H, int W);
int fd_pw_dw3x3_f32(const void *x, int ld_x, int off_x, int Cin, const float *ln_gamma, const float *ln_beta, float ln_eps,
                    const float *ln_shift, const float *ln_scale, int ln_ld, const void *w_pw_hi, const void *w_pw_lo, int Cdw,
                    const float *w_dw, const float *b_dw, int dw_silu, void *out_dw, int ld_dw, int off_dw, int B, int H, int W, void *stream);
int fd_pw_dw3x3_gram_f32_ok(int dtype, int Cin, int H, int W);
int fd_pw_dw3x3_gram_f32_nblk(int H, int W);
int fd_pw_dw3x3_gram_f32(const void *x, int ld_x, int off_x, int Cin, const float *ln_gamma, const float *ln_beta, float ln_eps,
                         const float *ln_shift, const float *ln_scale, int ln_ld, const void *w_pw_hi, const void *w_pw_lo,
                         const float *w_dw, int ld_wdw, float *partial, int B, int H, int W, void *stream);
int fd_pw_dw3x3_proj_f32_ok(int dtype, int Cin, int H, int W);
int fd_pw_dw3x3_proj_f32(const void *x, int ld_x, int off_x, int Cin, const float *ln_gamma, const float *ln_beta, float ln_eps,
                         const float *ln_shift, const float *ln_scale, int ln_ld, const void *w_pw_hi, const void *w_pw_lo,
                         const float *w_dw, int ld_wdw, const float *w2, const float *gate, int gate_ld, void *out, int ld_o, int off_o, int B,
                         int H, int W, void *stream);

/* ---- qkv_dwconv + L2 norms + q k^T for the wider blocks (C >= 128, src/DADiff.py:267-276): the depthwise 3x3 of the q
 * and k channels of a qkv tensor [B,H,W,ld] (q at channel 0, k at channel C) feeding the per-head Gram directly -- q and k
 * after the depthwise conv never reach HBM.  v keeps fd_dwconv3x3.  w_dw [9][3C/2] in fd_pw_dw3x3's fp16 layout;
 * partial [B][C/32][nblk][1024 + 64] in fd_chan_attn_gram's layout, nblk = fd_dwconv_gram_nblk(H, W).            */
int fd_dwconv_gram_ok(int dtype, int C, int H, int W);
int fd_dwconv_gram_nblk(int H, int W);
int fd_dwconv_gram(int dtype, const void *qkv, int ld, int C, const uint32_t *w_dw, float *partial, int B, int H, int W,
                   void *stream);

/* The launch plan of the seven entry points above.  Host only: touches no device.  Returns 1 and fills out[0 .. 8] when the matching
 * _ok query serves the shape, 0 (out untouched) otherwise; every launch runs exactly this plan.  entry = FD_PWDW_*; Cdw, Cz are read by
 * FD_PWDW_DW (Cdw also by FD_PWDW_F32), C by FD_PWDW_DWGRAM only.  Field order:
 *   [0] kernel, FD_PWDW_K_*   [1] tile width (tiles are 8 rows high)   [2] tiles per image   [3] tpw: consecutive tiles per workgroup
 *   [4] grid x = ceil(tiles / tpw): workgroup x walks tiles x * tpw .. ; equals the _nblk query of the Gram entries
 *   [5] grid y (images; fd_dwconv_gram: pairs of heads)   [6] grid z (fd_dwconv_gram: images)
 *   [7] 32-row groups of 1x1 weights per tile (pass-through groups first; 0 for fd_dwconv_gram)
 *   [8] depthwise chunks per tile (64 channels; 32 in the fp32-storage kernels)                                              */
#define FD_PWDW_DW 0          /* fd_pw_dw3x3 */
#define FD_PWDW_PROJ 1        /* fd_pw_dw3x3_proj */
#define FD_PWDW_GRAM 2        /* fd_pw_dw3x3_gram */
#define FD_PWDW_DWGRAM 3      /* fd_dwconv_gram */
#define FD_PWDW_F32 4         /* fd_pw_dw3x3_f32 */
#define FD_PWDW_GRAM_F32 5    /* fd_pw_dw3x3_gram_f32 */
#define FD_PWDW_PROJ_F32 6    /* fd_pw_dw3x3_proj_f32 */
#define FD_PWDW_K_64 0        /* pwdw_kernel<64> */
#define FD_PWDW_K_128 1       /* pwdw_kernel<128> */
#define FD_PWDW_K_64_PROJ 2   /* pwdw_kernel<64, PROJ> */
#define FD_PWDW_K_GRAM 3      /* pwdw_gram_kernel */
#define FD_PWDW_K_DWGRAM 4    /* dwconv_gram_kernel */
#define FD_PWDW_K_32_DW 5     /* pwdw32_kernel<DW, 16> */
#define FD_PWDW_K_32_GRAM 6   /* pwdw32_kernel<GRAM, 8> */
#define FD_PWDW_K_32_PROJ 7   /* pwdw32_kernel<PROJ, 8> */
int fd_pw_dw3x3_plan(int entry, int dtype_opts, int Cin, int Cdw, int Cz, int C, int B, int H, int W, int *out);

/* ---- SS2D selective scan (replaces selective_scan_cuda_core.fwd, src/emamba2.py:154, together
 * with EfficientScan/EfficientMerge index maps 182-262, dt_proj einsum 340, softplus/bias).
 *   xc    [B,H,W,D]    (dtype)  dwconv+SiLU output, D = d_inner = 2C
 *   xdbl  [4,B,L,CD]   fp32     x_proj output per direction, CD = R + 2N, row l' = h'*ceil(W/2) + w',
 *                               L = ceil(H/2)*ceil(W/2); odd H / W: the reference's zero padding (src/emamba2.py:
 *                               191-199, 253-260) -- rows of sub-grid positions outside the image must be zero
 *   dtw   [4,D,R], dtb [4,D], A [4*D,N] (= -exp(A_logs)), Ds [4*D]   fp32
 *   y     [B,H,W,D]    (dtype)  written at the merged pixel positions
 *   ws    fp32 workspace of fd_scan_ws_floats(...) floats
 * 3 phases over chunks of the sequence (L = H*W/4 per direction): local scan, carry scan,
 * final scan + C contraction + D skip.  fp32 state throughout.  Short sequences with a wide state
 * (L <= 1024, N >= 16, R % 8 == 0: the 64x64 level of a 512x512 slice) run ONE sequential pass instead, 4 lanes
 * per channel sharing the states and the dt_proj contraction -- no chunks, no workspace traffic; which form
 * runs depends on (H, W, N, R) only, never on B.                                              */
/* OR-ed into the `dtype` argument of fd_selective_scan / fd_selective_scan_plan: keep the chunked 3-phase form at every
 * size.  The single-pass form of short sequences is the faster one once a batch fills the chip (x1.7 at 8 slices of
 * 512x512) but walks its 1024 positions with one wave per channel group: a lone slice takes 2-3x longer in it.  An
 * engine uses ONE of the two for all its calls (DAEngine low_latency), so results stay batch-invariant within it.  */
#define FD_OPT_LOW_LATENCY 0x100
/* OR-ed into the `dtype` argument of fd_selective_scan_plan / fd_selective_scan_fuses_xproj / fd_selective_scan_xproj with
 * FD_F32 (round 6): the caller's fp32-storage engine runs its contractions split-bf16 (fd_conv_params.f32_split), so the
 * x_proj einsum (src/emamba2.py:332) may run inside the scan's first phase as three bf16 MFMAs per product, x_proj_w fp32
 * [4][R + 2N][d_inner].  Without it an FD_F32 scan takes its x_dbl rows from the workspace (exact parity mode).          */
#define FD_OPT_F32_SPLIT 0x200
int64_t fd_scan_ws_floats(int B, int H, int W, int D, int N);
int fd_selective_scan(int dtype, const void *xc, const float *xdbl, const float *dtw,
                      const float *dtb, const float *A, const float *Ds, void *y, float *ws,
                      int B, int H, int W, int D, int N, int R, void *stream);
/* The same scan with the x_proj einsum (src/emamba2.py:332) folded into its first phase: x_proj_w [4][R+2N][D] in
 * dtype; xdbl is then an OUTPUT workspace (phase A writes the rows phase C reads).  Saves the separate x_proj
 * launch and its pass over xc.  Only where fd_selective_scan_fuses_xproj() says so (bf16, d_inner <= 256).     */
int fd_selective_scan_fuses_xproj(int dtype, int D, int N, int R);
int fd_selective_scan_xproj(int dtype, const void *xc, const void *x_proj_w, float *xdbl, const float *dtw,
                            const float *dtb, const float *A, const float *Ds, void *y, float *ws, int B, int H,
                            int W, int D, int N, int R, void *stream);
/* 1: call fd_selective_scan_xproj for this block; 0: run the x_proj launch, then fd_selective_scan (the single-pass
 * form takes its x_dbl rows from the workspace).                                                              */
int fd_selective_scan_plan(int dtype, int D, int N, int R, int H, int W);
/* Which device code a call of fd_selective_scan (fused = 0) or fd_selective_scan_xproj (fused = 1) with this dtype (options
 * included) and shape runs -- the launcher's own decisions, host only, a function of the shape and never of B:
 *   out[0] form: 0 single-pass, 1 chunked; for the single-pass form out[1..7] are 0
 *   out[1] chunk length            out[2] number of chunks
 *   out[3] channels per lane (1, 2) out[4] waves per workgroup      out[5] workgroups per chunk
 *   out[6] carry kernel: -1 none (a single chunk), else chunks per segment held in registers (2, 8) or 0 (two passes)
 *   out[7] dynamic LDS bytes of the chunk kernel
 * Returns what the call itself would return for the shape: an error for an unsupported one, also where the chunk kernel
 * would need more than 64 KiB of LDS (N = 32 in 256-step chunks, d_inner * L >= 2^24; out is filled all the same).     */
int fd_selective_scan_geom(int dtype, int fused, int D, int N, int R, int H, int W, int32_t out[8]);

/* ---- The reference's own native-op interface (the only one it has):
 *     out, x, *rest = selective_scan_cuda_core.fwd(u, delta, A, B, C, D, delta_bias, delta_softplus, nrows)
 * /root/reference/src/emamba2.py:154, layout asserted at 124-149.  All tensors fp32, contiguous in the last dim:
 *   u, delta [batch,KD,L]   A [KD,N]   B, C [batch,K,N,L] (K groups, channel d uses group d / (KD/K))
 *   D, delta_bias [KD] (either may be NULL)      out [batch,KD,L]
 *   x_last [batch,KD,N] or NULL: the state after the last position (the extension's second return value holds
 *   the chunk states its backward pass needs; this library is forward-only and returns the final state instead)
 * nrows is the extension's rows-per-block tuning knob: validated like the reference does (1..4, KD % (K*nrows)
 * == 0, src/emamba2.py:129-130) and otherwise without effect.  Python shim with the extension's module and
 * function name: founddiff_amd/selective_scan_cuda_core.py.                                                 */
int fd_selective_scan_fwd_f32(const float *u, const float *delta, const float *A, const float *B,
                              const float *C, const float *D, const float *delta_bias, int delta_softplus,
                              int nrows, int batch, int KD, int K, int N, int64_t L, float *out, float *x_last,
                              void *stream);
/* Its backward (selective_scan_cuda_core.bwd, src/emamba2.py:172): the same operands plus dout [batch,KD,L]; writes
 *   du, ddelta [batch,KD,L]   dA [KD,N]   dB, dC [batch,K,N,L]   dD, ddelta_bias [KD] (NULL exactly when D / delta_bias are)
 * No forward state is read: h and dL/dh are recomputed from tile carries the call computes itself (fd_scan_bwd.hip).
 * Deterministic (fixed-order reductions, no float atomics).  ws: fd_selective_scan_bwd_ws_floats(...) floats, 16-byte
 * aligned.  nrows, K and alignment are validated as in the forward.                                           */
int64_t fd_selective_scan_bwd_ws_floats(int batch, int KD, int K, int N, int64_t L);
int fd_selective_scan_bwd_f32(const float *u, const float *delta, const float *A, const float *B, const float *C,
                              const float *D, const float *delta_bias, const float *dout, int delta_softplus, int nrows,
                              int batch, int KD, int K, int N, int64_t L, float *du, float *ddelta, float *dA, float *dB,
                              float *dC, float *dD, float *ddelta_bias, float *ws, void *stream);
/* What that call launches for a shape -- the launcher's own layout, host only:
 *   out[0] tiles of 256 positions   out[1] carry workgroups per row (4 tiles each)   out[2] length of the last tile
 *   out[3] row splits S per (batch, group, tile)   out[4] states per chunk of the main kernel (4, 8)
 *   out[5] rows of the largest split   out[6] rows per group KD / K   out[7] 0
 * Returns what the call returns for the shape (with nrows = 1): an error, and out all 0, for a refused one.        */
int fd_selective_scan_bwd_geom(int batch, int KD, int K, int N, int64_t L, int32_t out[8]);

/* ---- The reference's cross_selective_scan (src/emamba2.py:295-367) up to out_norm, for training, fp32 (fd_cross_scan_bwd.hip).
 * Forward: x [B,D,H,W] (NCHW, forward_corev2's layout) -> xc [B,H,W,D] (NHWC), the x_proj gather as fd_conv2d with ndir = 4
 * (exact fp32) -> xdbl [4,B,L,CD], fd_selective_scan in FD_F32 -> y [B,H,W,D] at the merged pixels.  Operands as for
 * fd_selective_scan: x_proj_w [4][CD][D], dtw [4,D,R], dtb [4,D], A [4*D,N] (= -exp(A_logs)), Ds [4*D]; ws: fd_scan_ws_floats(...)
 * floats.  xc and xdbl are everything the backward reads of the forward.
 * Backward: dy [B,H,W,D] (the gradient of y) -> dx [B,D,H,W] (NCHW), dx_proj_w [4][CD][D], ddtw [4,D,R], ddtb [4,D], dA [4*D,N],
 * dDs [4*D], all written (not accumulated).  The selective-scan gradients of fd_selective_scan_bwd_f32 on the gathered
 * operands, the dt_proj and x_proj einsums' backwards and the gather / merge as index maps: no activation-sized tensor is
 * written besides dx.  Odd H / W: the padded positions take part with u = 0, a zero x_dbl row and dy = 0, as in the
 * reference's EfficientScan / EfficientMerge (src/emamba2.py:191-199, 253-260).  Deterministic (fixed-order sums, no float
 * atomics); tile sizes, channel splits and reduction orders depend on (H, W, D, N, R) only, so a slice's dx is the same bits
 * alone or in a batch.  ws: fd_cross_scan_bwd_ws_floats(...) floats, 0 for an unsupported shape.  D % 64 == 0,
 * N in {4, 8, 16, 32}, R in {2, 4, 8, 16, 32}, B <= 16383 (batch x direction is a grid.y); xc, dy, ws 16-byte aligned.       */
int fd_cross_scan_fwd_f32(const float *x, const float *x_proj_w, const float *dtw, const float *dtb, const float *A,
                          const float *Ds, float *xc, float *xdbl, float *y, float *ws, int B, int H, int W, int D, int N,
                          int R, void *stream);
int64_t fd_cross_scan_bwd_ws_floats(int B, int H, int W, int D, int N, int R);
/* What the backward (either layout) launches for a shape -- the launcher's own layout, host only, of B only the validity:
 *   out[0] positions per lane E (4 where R + 2N <= 24, else 1)   out[1] tile length 64 E   out[2] L = ceil(H/2) ceil(W/2)
 *   out[3] tiles   out[4] length of the last tile   out[5] channel splits S   out[6] x_proj blocks of 256 rows
 *   out[7] static LDS bytes of the larger of the scan and the x_proj kernel
 * Returns what the call returns for the shape: an error, and out all 0, for a refused one.                           */
int fd_cross_scan_bwd_geom(int B, int H, int W, int D, int N, int R, int32_t out[8]);
int fd_cross_scan_bwd_f32(const float *xc, const float *xdbl, const float *x_proj_w, const float *dtw, const float *dtb,
                          const float *A, const float *Ds, const float *dy, float *dx, float *dx_proj_w, float *ddtw,
                          float *ddtb, float *dA, float *dDs, float *ws, int B, int H, int W, int D, int N, int R,
                          void *stream);

/* The same two with NHWC on both sides, for callers that already hold the activation channel-last (fd_ss2d_train.hip's
 * neighbours): the forward takes xc [B,H,W,D] itself (no layout launch; xdbl, y and ws as above), the backward writes
 * dxc [B,H,W,D] (16-byte aligned) in place of dx -- du leaves through the LDS slab that brought u in, 16 bytes per (pixel,
 * 4 channels), and the x_proj term is added with lane = channel.  Everything else, the workspace included, as above.       */
int fd_cross_scan_fwd_nhwc_f32(const float *xc, const float *x_proj_w, const float *dtw, const float *dtb, const float *A,
                               const float *Ds, float *xdbl, float *y, float *ws, int B, int H, int W, int D, int N, int R,
                               void *stream);
int fd_cross_scan_bwd_nhwc_f32(const float *xc, const float *xdbl, const float *x_proj_w, const float *dtw, const float *dtb,
                               const float *A, const float *Ds, const float *dy, float *dxc, float *dx_proj_w, float *ddtw,
                               float *ddtb, float *dA, float *dDs, float *ws, int B, int H, int W, int D, int N, int R,
                               void *stream);

/* ---- The rest of SS2D.forward (src/emamba2.py:713-751) around the scan, for training, fp32, NHWC (fd_ss2d_train.hip).  The
 * operands are the halves of in_proj's output xz [B,H,W,2D] and of its gradient, read and written in place through a pixel
 * stride (ld) and a channel offset (off).  Deterministic (per-workgroup partials summed in a fixed order, no float atomics);
 * tile sizes and the order of every per-slice sum depend on (H, W, C) only.  C % 64 == 0; pointers 16-byte aligned.
 *
 * fd_dwconv3x3_silu_bwd_f32: backward of xc = SiLU(dwconv3x3(x) + bias), fd_dwconv3x3(FD_F32, ..., silu = 1)'s forward.
 *   x [B,H,W,ld_in] channels [off_in, +C); weight [9][C] tap-major and bias [C] or NULL as fd_dwconv3x3 takes them;
 *   dout [B,H,W,C] dense, the gradient of xc: OVERWRITTEN with the gradient of the pre-activation (which is recomputed from
 *   x, not stored by the forward); dx [B,H,W,ld_dx] channels [off_dx, +C), the other channels untouched; dweight [9][C];
 *   dbias [C], NULL exactly when bias is.  Zero padding at the border as the forward.  ld / off multiples of 8.
 *   ws: fd_dwconv3x3_silu_bwd_ws_floats(...) floats, 0 for an unsupported shape.
 * fd_ln_silu_gate_fwd_f32: out = LN(y) * SiLU(z) + local[b]  (out_norm, * act(z), + local: src/emamba2.py:365, 720, 747-748).
 *   fd_ln_gate with the activation of z inside.  y, out [B,hw,C] dense; z [B,hw,ldz] channels [offz, +C) (the z half of
 *   xz, NOT activated); local [B][local_ld] or NULL; stats [B,hw,2] receives (mean, rstd) per pixel for the backward.
 *   C <= 1024; ld / off multiples of 4.
 * fd_ln_silu_gate_bwd_f32: dout [B,hw,C] -> dy [B,hw,C] dense, dz [B,hw,lddz] channels [offdz, +C) (the z half of dxz),
 *   dgamma [C], dbeta [C], dlocal [B][C] (the sum of dout over the slice's pixels) or NULL.  Reads y, z and stats; nothing
 *   else of the forward.  ws: fd_ln_silu_gate_bwd_ws_floats(...) floats, 0 for an unsupported shape.                       */
int64_t fd_dwconv3x3_silu_bwd_ws_floats(int B, int H, int W, int C);
int fd_dwconv3x3_silu_bwd_f32(const float *x, int ld_in, int off_in, const float *weight, const float *bias, float *dout,
                              float *dx, int ld_dx, int off_dx, float *dweight, float *dbias, float *ws, int B, int H, int W,
                              int C, void *stream);
int fd_ln_silu_gate_fwd_f32(const float *y, const float *gamma, const float *beta, float eps, const float *z, int ldz, int offz,
                            const float *local, int local_ld, float *out, float *stats, int B, int64_t hw, int C,
                            void *stream);
int64_t fd_ln_silu_gate_bwd_ws_floats(int B, int64_t hw, int C);
int fd_ln_silu_gate_bwd_f32(const float *dout, const float *y, const float *stats, const float *gamma, const float *beta,
                            const float *z, int ldz, int offz, float *dy, float *dz, int lddz, int offdz, float *dgamma,
                            float *dbeta, float *dlocal, float *ws, int B, int64_t hw, int C, void *stream);

/* ---- The core of TransposedAttention.forward (src/DADiff.py:263-285) for training, fp32, NHWC (fd_tattn_train.hip, and
 * fd_dwconv3x3_bwd_f32 in fd_ss2d_train.hip).  q, k, v are the three C-wide thirds of qkv [B,hw,ld] channels [off, +3C), read in
 * place; heads are 32 channels wide (heads = C / 32); per (b, head), i and j run over the head's channels.  Deterministic (Gram
 * partials per pixel block summed in a fixed order, no float atomics); the block size and the order of every per-slice sum
 * depend on (hw, C) only.  C % 64 == 0, C <= 512; ld / off multiples of 4; pointers 16-byte aligned.
 *
 * fd_chan_attn_fwd_f32: G = q^T k over the pixels, nq / nk = max(column norm, 1e-12) (F.normalize), ghat = G / (nq nk^T),
 *   attn = softmax_j(ghat * temperature[head]) with expf-accuracy exponentials, out[p,i] = sum_j attn[i][j] v[p,j].
 *   temperature [heads]; out [B,hw,C] dense; attn, ghat [B][heads][32][32]; nrm [B][heads][64] (nq then nk): the three small
 *   tensors are all the backward needs beyond qkv.  ws: fd_chan_attn_fwd_ws_floats(...) floats, 0 for an unsupported shape.
 * fd_chan_attn_bwd_f32: dout [B,hw,C] dense -> dqkv [B,hw,ld_d] channels [off_d, +3C) (dq | dk | dv, the other channels
 *   untouched) and dtemperature [heads] (summed over the batch in order).  Three launches over the activation: a Gram pass over
 *   dout and v, a per-(b, head) kernel, one pass that reads q, k, dout and writes dqkv.
 *   ws: fd_chan_attn_bwd_ws_floats(...) floats, 0 for an unsupported shape.
 * fd_dwconv3x3_bwd_f32: backward of y = dwconv3x3(x) + bias, fd_dwconv3x3(FD_F32, ..., silu = 0)'s forward (qkv_dwconv):
 *   fd_dwconv3x3_silu_bwd_f32 without the activation, same operands, but dout [B,H,W,C] is only read.  C % 64 == 0 (3 * 512 =
 *   1536 included); ld / off multiples of 8.  ws: fd_dwconv3x3_bwd_ws_floats(...) floats, 0 for an unsupported shape.          */
int64_t fd_chan_attn_fwd_ws_floats(int B, int64_t hw, int C);
int fd_chan_attn_fwd_f32(const float *qkv, int ld, int off, const float *temperature, float *out, float *attn, float *ghat,
                         float *nrm, float *ws, int B, int64_t hw, int C, void *stream);
int64_t fd_chan_attn_bwd_ws_floats(int B, int64_t hw, int C);
int fd_chan_attn_bwd_f32(const float *qkv, int ld, int off, const float *temperature, const float *attn, const float *ghat,
                         const float *nrm, const float *dout, float *dqkv, int ld_d, int off_d, float *dtemperature, float *ws,
                         int B, int64_t hw, int C, void *stream);
int64_t fd_dwconv3x3_bwd_ws_floats(int B, int H, int W, int C);
int fd_dwconv3x3_bwd_f32(const float *x, int ld_in, int off_in, const float *weight, const float *bias, const float *dout,
                         float *dx, int ld_dx, int off_dx, float *dweight, float *dbias, float *ws, int B, int H, int W, int C,
                         void *stream);

/* ---- The element-wise frame of Mamba_block.forward (src/DADiff.py:477-488) for training, fp32, NHWC (fd_adaln_train.hip):
 * LayerNorm + modulate in front of a branch, the gated residual add behind it.  x, y, out and the gradients [B,hw,C] dense;
 * shift, scale, gate [B][ld_mod] (the chunks of adaLN_modulation's [B,6C] output, read in place: 16-byte aligned, ld_mod a
 * multiple of 4); their gradients [B][ld_dmod], only the C columns written.  Deterministic (a workgroup owns a contiguous pixel
 * range whose length depends on hw only, partials summed in a fixed order, no float atomics): every per-slice result is the
 * same bits alone or in a batch; dgamma and dbeta add the slices in index order.  C % 64 == 0, C <= 512.
 *
 * fd_adaln_fwd_f32: out = LN(x) * (1 + scale[b]) + shift[b].  gamma, beta [C], both set or both NULL (no affine); stats
 *   [B,hw,2] receives (mean, rstd) per pixel; centred statistics (the variance of x - mean).
 * fd_adaln_bwd_f32: dout -> dx, dshift, dscale, dgamma, dbeta (NULL exactly when gamma is).  dres [B,hw,C] or NULL is added to
 *   dx in the same pass: the gradient that reaches x along the residual path.  Reads dout, x, stats, dres once; dout and x are
 *   not modified.  ws: fd_adaln_bwd_ws_floats(...) floats, 0 for an unsupported shape.
 * fd_gate_res_fwd_f32: out = x + gate[b] * y.
 * fd_gate_res_bwd_f32: dy = gate[b] * dout, dgate[b,c] = sum over the pixels of dout * y.  The gradient of x is dout itself and
 *   is not written.  ws: fd_gate_res_bwd_ws_floats(...) floats, 0 for an unsupported shape.                                    */
int fd_adaln_fwd_f32(const float *x, const float *gamma, const float *beta, float eps, const float *shift, const float *scale,
                     int ld_mod, float *out, float *stats, int B, int64_t hw, int C, void *stream);
int64_t fd_adaln_bwd_ws_floats(int B, int64_t hw, int C);
int fd_adaln_bwd_f32(const float *dout, const float *x, const float *stats, const float *gamma, const float *beta,
                     const float *scale, int ld_mod, const float *dres, float *dx, float *dshift, float *dscale, int ld_dmod,
                     float *dgamma, float *dbeta, float *ws, int B, int64_t hw, int C, void *stream);
int fd_gate_res_fwd_f32(const float *x, const float *y, const float *gate, int ld_mod, float *out, int B, int64_t hw, int C,
                        void *stream);
int64_t fd_gate_res_bwd_ws_floats(int B, int64_t hw, int C);
int fd_gate_res_bwd_f32(const float *dout, const float *y, const float *gate, int ld_mod, float *dy, float *dgate, int ld_dmod,
                        float *ws, int B, int64_t hw, int C, void *stream);

/* ---- The backward of the reference's ResnetBlock (src/DADiff.py:139-154, 213-229, 397-430) for training, fp32, NHWC
 * (fd_resblock_train.hip): out = SiLU(GroupNorm(h)) (+ res) with h = conv3x3(x, w) + bias.  The forward is fd_conv2d(FD_F32) with
 * stats_partial, fd_gn_finalize and fd_gn_silu_apply; the gradient of res is dout itself; the gradient of x is fd_conv2d(FD_F32)
 * over dh with the weight wd[c][kh][kw][n] = w[n][2-kh][2-kw][c].  Deterministic (per-workgroup partials summed in a fixed order,
 * no float atomics); chunk and tile sizes, the split count and every order of summation depend on the shape only, and nothing in
 * one slice's dh depends on the batch.  Pointers 16-byte aligned.
 *
 * fd_gn_silu_bwd_f32: dout [B,hw,C] (the gradient of out) and the raw convolution output h [B,hw,C], both only read; mean_rstd
 *   [B][groups][2] as fd_gn_finalize leaves it; gamma, beta [C].  -> dh [B,hw,C] (the gradient of h), dgamma, dbeta [C] and
 *   dbias [C] or NULL (the sum of dh over batch and pixels: the convolution's bias gradient).  The SiLU input is recomputed, not
 *   stored.  C % 32 == 0, C <= 512, C % groups == 0, (C / groups) % 4 == 0.
 *   ws: fd_gn_silu_bwd_ws_floats(...) floats, 0 for an unsupported shape.
 * fd_conv3x3_wgrad_f32: dw[n][kh][kw][c] = sum over (b, y, x) of dh[b,y,x,n] x[b,y+kh-1,x+kw-1,c] with zero padding, in
 *   fd_conv2d's weight layout [Cout][9 Cin], on the exact-f32 MFMA.  x [B,H,W,ld_x] channels [off_x, +Cin); dh [B,H,W,Cout]
 *   dense; dw written, not accumulated.  The pixels are split over workgroups, whose partial results go to ws and are added in
 *   order.  Cin % 16 == 0, Cin <= 1024; Cout % 32 == 0, Cout <= 512; ld_x / off_x multiples of 4.
 *   ws: fd_conv3x3_wgrad_ws_floats(...) floats, 0 for an unsupported shape.                                                  */
int64_t fd_gn_silu_bwd_ws_floats(int B, int64_t hw, int C, int groups);
int fd_gn_silu_bwd_f32(const float *dout, const float *h, const float *mean_rstd, const float *gamma, const float *beta,
                       float *dh, float *dgamma, float *dbeta, float *dbias, float *ws, int B, int64_t hw, int C, int groups,
                       void *stream);
int64_t fd_conv3x3_wgrad_ws_floats(int B, int H, int W, int Cin, int Cout);
int fd_conv3x3_wgrad_f32(const float *x, int ld_x, int off_x, const float *dh, float *dw, float *ws, int B, int H, int W, int Cin,
                         int Cout, void *stream);

/* ---- The resampling convolutions of the U-Net (src/DADiff.py:128-136) for training, fp32, NHWC (fd_resample_train.hip).  Down =
 * Conv2d(4, stride 2, pad 1), Up = nearest x2 -> Conv2d(3, pad 1); each is the other's transpose up to a fixed fold of the taps, so
 * these two and fd_conv2d(FD_F32) cover the forward and every gradient of both (founddiff_amd/resample_train.py).  Exact-f32 MFMA,
 * deterministic (no float atomics; tile sizes, the split count and every order of summation depend on the shape only).  Channel
 * counts multiples of 32, at most 512; tensors dense, pointers 16-byte aligned; anything else fails with FD_ERR_ARG.
 *
 * fd_conv_sub2x_f32: in [B,H,W,Cin] -> out [B,2H,2W,Cout], w2 [Cout][4][2][2][Cin], bias [Cout] or NULL:
 *     out[b, 2i+a, 2j+b', n] = bias[n] + sum_{r,s,c} w2[n][2a+b'][r][s][c] in[b, i+a+r-1, j+b'+s-1, c],  r, s in {0, 1},
 *   zero outside `in`: output pixel (2i+a, 2j+b') reads source pixels (i+a+r-1, j+b'+s-1).  The Up forward takes the 3x3 taps that
 *   land on one source pixel summed, the layout of fd_conv_params.weight_up2x (a = 0: r = 0 <- kh 0, r = 1 <- kh 1 + 2; a = 1:
 *   r = 0 <- kh 0 + 1, r = 1 <- kh 2; columns likewise).  The input gradient of Down has the same index map with no summing:
 *   dx[2i+a, 2j+b', c] = sum_{r,s,n} dout[i+a+r-1, j+b'+s-1, n] w[n, c, kh(a,r), kw(b',s)] with kh(0,0) = 3, kh(0,1) = 1,
 *   kh(1,0) = 2, kh(1,1) = 0 and kw likewise, i.e. w2[c][2a+b'][r][s][n] = w[n][c][kh(a,r)][kw(b',s)].  One slice's result does not
 *   depend on the batch.
 * fd_corr4x4s2_f32: coarse [B,H,W,P], fine [B,2H,2W,Q] -> g [P][4][4][Q], written, not accumulated:
 *     g[p][t][u][q] = sum_{b,i,j} coarse[b,i,j,p] fine[b, 2i+t-1, 2j+u-1, q],  zero outside `fine`.
 *   Down's weight gradient is coarse = dout, fine = x: dweight[n][kh][kw][c] in fd_conv2d's weight layout.  Up's is coarse = x,
 *   fine = dout, then dweight[n][c][kh][kw] = sum_{t in {2-kh, 3-kh}} sum_{u in {2-kw, 3-kw}} g[c][t][u][n].  The coarse pixels
 *   are split over workgroups, whose partial results go to ws and are added in order; one split writes g directly.
 *   ws: fd_corr4x4s2_ws_floats(...) floats, 0 for an unsupported shape.                                                      */
int fd_conv_sub2x_f32(const float *in, const float *w2, const float *bias, float *out, int B, int H, int W, int Cin, int Cout,
                      void *stream);
int64_t fd_corr4x4s2_ws_floats(int B, int H, int W, int P, int Q);
int fd_corr4x4s2_f32(const float *coarse, const float *fine, float *g, float *ws, int B, int H, int W, int P, int Q, void *stream);

/* ---- channel ("transposed") attention, src/DADiff.py:263-285 ------------------------------
 * fd_chan_attn_gram: per (b, head) partial 32x32 Gram q^T k and sums of squares over pixel
 *   blocks.  qkv [B,HW,3C] (dtype).  partial: fp32 [B][heads][nblk][32*32+64].
 * fd_chan_attn_weff: reduce partials, L2-normalise, *temperature, softmax, and fold the
 *   result into project_out:  Weff[b][o][h*32+j] = sum_i Wp[o][h*32+i] * attn[b,h,i,j]
 *   so that attn@v followed by project_out is ONE GEMM over v (fd_conv2d, w_batch_stride).   */
int fd_chan_attn_nblk(int64_t hw);
int fd_chan_attn_gram(int dtype, const void *qkv, int B, int64_t hw, int C, float *partial,
                      void *stream);
/* (`partial` is reduced IN PLACE over the pixel blocks: slot 0 of each (b, head) holds the sums) */
int fd_chan_attn_weff(int dtype, float *partial, int nblk, const float *temperature,
                      const float *wproj /* [C][C] fp32 */, void *weff /* [B][C][C] dtype */,
                      int B, int C, void *stream);

/* ---- small fp32 dense layers and conditioning ---------------------------------------------
 * fd_linear: out[m,n] = act(b[n] + sum_k x[m,k] w[n,k]);  act: 0 none, 1 SiLU, 2 GELU(erf),
 *   3 ReLU.  pre_silu: apply SiLU to x first (adaLN_modulation = Linear(SiLU(t))).
 *   time MLP (src/DADiff.py:580-585), text/prompt MLPs (606-611), adaLN (463-466),
 *   SS2D `attn` (src/emamba2.py:522-525), DA-CLIP heads (src/DACLIP.py:1179-1188).           */
int fd_linear(const float *x, const float *w, const float *b, float *out, int M, int N, int K,
              int act, int pre_silu, void *stream);
/* sinusoidal embedding, src/DADiff.py:173-185: out[b] = [sin(t f_i), cos(t f_i)]             */
int fd_sinusoidal(const float *time, float *out, int B, int dim, void *stream);
/* out = softmax(x, dim=1) * p[n]   (prompt path, src/DADiff.py:706)                         */
int fd_softmax_mul(const float *x, const float *p, float *out, int M, int N, void *stream);
/* out = x / max(||x||_2, eps) per row                                                       */
int fd_l2norm_rows(const float *x, float *out, int M, int N, float eps, void *stream);
int fd_add_f32(const float *a, const float *b, float *out, int64_t n, void *stream);

/* ---- image <-> activation glue ------------------------------------------------------------
 * fd_pack_planes: NCHW fp32 planes -> NHWC `cpad` channels (dtype), zero padded
 *   (torch.cat((x, x_input), 1) src/DADiff.py:1160; x[:,1].repeat(1,3,..) 692 is folded).    */
int fd_pack_planes(int dtype, const float *p0, const float *p1, void *out, int B, int64_t hw,
                   int cpad, void *stream);
/* fd_init_conv7: the UNet's init_conv (7x7, pad 3, bias) straight from the fp32 image planes
 *   (src/DADiff.py:558, 704) -- bf16 mode, Cout in {32, 64}, H and W multiples of 16
 *   (fd_init_conv7_ok; otherwise fd_pack_planes3 + fd_conv2d).
 *   p0, p1, p2: [B,H,W] fp32 planes (x_t, x_input, x_input_condition; p1 / p2 may be NULL)
 *   w_packed: bf16 [Cout][7 kh][8 kw][4 c], zero where kw = 7 or c >= number of planes -- except
 *             that with p2 == NULL slots c = 2, 3 must repeat the weights of planes 0, 1: the kernel
 *             feeds them the bf16 rounding residuals of the two planes (hi + lo split)
 *   out: [B,H,W,Cout] bf16                                                                    */
int fd_init_conv7_ok(int dtype, int Cout, int H, int W);
int fd_init_conv7(int dtype, const float *p0, const float *p1, const float *p2, const void *w_packed,
                  const float *bias, void *out, int B, int H, int W, int Cout, void *stream);
/* The same layer on fp32 storage with the split-bf16 contraction of the `fp32s` engine (round 6), two input planes, fp32 out:
 * w_hi_packed = fd_init_conv7's packing of bf16(w) (all four channel slots: planes and their bf16 rounding residuals),
 * w_lo_packed = the same packing of bf16(w - bf16(w)) with slots 2, 3 zero: w_hi.x_hi + w_hi.x_lo + w_lo.x_hi.         */
int fd_init_conv7_f32s(const float *p0, const float *p1, const void *w_hi_packed, const void *w_lo_packed, const float *bias,
                       void *out, int B, int H, int W, int Cout, void *stream);
/* same with a third plane: torch.cat((x, x_input, x_input_condition), 1)  src/DADiff.py:1157-1158
 * (p1, p2 may be NULL)                                                                        */
int fd_pack_planes3(int dtype, const float *p0, const float *p1, const float *p2, void *out, int B,
                    int64_t hw, int cpad, void *stream);
/* final 1x1 conv to ONE channel (src/DADiff.py:683,740): out[b,p] = b0 + sum_c x[b,p,c] w[c] */
/* n elements (n % 8 == 0) of an activation tensor from one storage type to the other (FD_F32 <-> FD_BF16): the
 * level boundary of a hybrid-precision forward (engine.py: DAEngine.forward_hybrid).                       */
int fd_cast(int src_dtype, const void *in, int dst_dtype, void *out, int64_t n, void *stream);
int fd_final_conv1(int dtype, const void *x, const float *w, const float *b, float *out,
                   int64_t npix, int C, void *stream);
/* avg-pool k x k stride k, NHWC (src/DACLIP.py:181,193,282)                                  */
int fd_avgpool(int dtype, const void *in, void *out, int B, int H, int W, int C, int k,
               void *stream);
/* attention-pool helpers (src/DACLIP.py:226-259): tokens = [mean; x]  ->  [B, HW+1, C]      */
int fd_attnpool_tokens(int dtype, const void *x, void *tok, int B, int64_t hw, int C,
                       void *stream);
/* one-query multi-head attention: q rows of stride q_ld, k/v [B,T,ld] fp32 -> out [B,C] fp32 */
int fd_attnpool_core(const float *q, int q_ld, const float *kv, int ld, int koff, int voff, float *out,
                     int B, int T, int C, int heads, void *stream);

/* ---- scheduler math (fp32 images, shape [B, npix]) ----------------------------------------
 * fd_res_predictions: pred_res = clamp(out); pred_noise = (x_t - x_in - (ac-1) pred_res)/bc;
 *   x_start = clamp(x_in - pred_res)          src/DADiff.py:1202-1207, 1120-1124
 *   ac, bc: per-batch alphas_cumsum[t], betas_cumsum[t] (device, [B]).                       */
int fd_res_predictions(const float *model_out, const float *x_t, const float *x_in,
                       const float *ac, const float *bc, float *pred_res, float *pred_noise,
                       float *x_start, int B, int64_t npix, void *stream);
/* fd_res_ddim_step: img' = last ? clamp(x_in - clamp(out)) : img - alpha*clamp(out) + sigma*noise
 *   src/DADiff.py:1317-1318, 1344 (type "use_pred_noise").  noise may be NULL (eta = 0).     */
int fd_res_ddim_step(const float *model_out, const float *img, const float *x_in,
                     const float *noise, float alpha, float sigma, int last, float *img_out,
                     int64_t n, void *stream);
/* fd_res_step_obj: the same three operations for every objective of model_predictions
 *   (src/DADiff.py:1168-1207) and the dual-UNet model (817-836).
 *   mode 0: o0 = residual (pred_res; pred_res_noise tested as "res")
 *        1: o1 = noise    (pred_noise; pred_res_noise tested as "noise"): x_start =
 *           clamp((x_t - ac x_in - bc o1)/omac), pred_res = clamp(x_in - x_start)      1126-1130
 *        2: o0 = residual, o1 = noise: x_start = clamp(x_t - ac clamp(o0) - bc o1)     1132-1136
 *        3: o0 = x_0, o1 = noise (pred_x0_noise): pred_res = clamp(x_in - o0)          1191-1195
 *   par [B][8] = {ac, bc, omac, k0, k1, k2, k3, flag} (alphas_cumsum[t], betas_cumsum[t],
 *        one_minus_alphas_cumsum[t] per batch element)
 *   step 0: predictions only (any of pred_res / pred_noise / x_start may be NULL)
 *        1: DDIM: img_out = flag ? x_start : x_t - k0 pred_res + k1 noise             1317-1318, 1344
 *        2: posterior: img_out = k0 x_t + k1 pred_res + k2 x_start + exp(k3/2) noise  1142-1151, 1226-1229
 *   noise may be NULL.                                                                        */
int fd_res_step_obj(int mode, int step, const float *o0, const float *o1, const float *x_t,
                    const float *x_in, const float *noise, const float *par, float *pred_res,
                    float *pred_noise, float *x_start, float *img_out, int B, int64_t npix,
                    void *stream);
/* fd_res_posterior_step: mean = c1 x_t + c2 pred_res + c3 x_start; out = mean + exp(.5 lv) noise
 *   src/DADiff.py:1142-1151, 1226-1229.  coef: [B][4] = c1,c2,c3,logvar.  noise NULL at t=0. */
int fd_res_posterior_step(const float *model_out, const float *x_t, const float *x_in,
                          const float *noise, const float *coef, float *img_out,
                          float *x_start_out, int B, int64_t npix, void *stream);
/* ---- ancestral sampling without a host in the loop, step noise keyed per slice (fd_sched.hip)
 * The reference draws randn_like(x) from the device generator at every step (src/DADiff.py:1228): a slice's noise
 * depends on its place in the batch.  Here noise(slice, t, pixel) = Box-Muller(Philox4x32-10(key = seeds[b] (64 bit),
 * counter = (pixel / 4, t, 0x46444e5a, 0))): the same slice gets the same stream on any rank / batch / stream
 * (BASELINE configs[3]: a volume sharded over 8 GPUs).  oracle/keyed_noise.py restates it.
 *   fd_keyed_normal               out[b][i] = that noise (x_T draws with t = 0x7fffffff, tests)
 *   fd_ancestral_begin            *t_dev -= 1;  time_buf[b] = times[*t_dev]   (times = alphas_cumsum * T, device)
 *   fd_res_posterior_step_keyed   fd_res_posterior_step with t = *t_dev, coefficients coef_table[t][4] = c1, c2, c3,
 *                                 logvar (device, [T][4]) and the keyed noise (none at t = 0)
 * All three read the step from DEVICE memory: a chunk of steps captures into one HIP graph.                   */
int fd_keyed_normal(const int64_t *seeds, int t, float *out, int B, int64_t npix, void *stream);
int fd_ancestral_begin(int *t_dev, const float *times, float *time_buf, int B, void *stream);
int fd_res_posterior_step_keyed(const float *model_out, const float *x_t, const float *x_in,
                                const float *coef_table, const int *t_dev, const int64_t *seeds,
                                float *img_out, float *x_start_out, int B, int64_t npix, void *stream);
/* ---- the same two for every objective of model_predictions and the two-U-Net model (fd_sched.hip), fp32
 * The ancestral step of fd_res_step_obj (step == 2, modes 0-3 as above) with nothing of the step on the host:
 *   fd_obj_begin            t = *t_dev = min(max(*t_dev - 1, 0), T - 1);  time0[b] = times0[t], time1[b] = times1[t]  (b < B)
 *                           times0 / times1: device tables [T] of the two U-Nets' time inputs (alphas_cumsum * T or
 *                           betas_cumsum * T for unet0, betas_cumsum * T for unet1).  time0 or time1 may be NULL -- the plan
 *                           does not run that U-Net -- and is then left alone (its table may be NULL too).
 *   fd_res_step_obj_keyed   t = *t_dev (held in [0, T)); par_table [T][8], row t = {ac, bc, omac, c1, c2, c3, logvar, 0}
 *                           (alphas_cumsum[t], betas_cumsum[t], one_minus_alphas_cumsum[t], posterior_mean_coef1..3[t],
 *                           posterior_log_variance_clipped[t]), the same row for every slice;
 *                             mode 0: pred_res = clamp(o0), x_start = clamp(x_in - pred_res)
 *                                  1: x_start = clamp((x_t - ac x_in - bc o1) / omac), pred_res = clamp(x_in - x_start)
 *                                  2: pred_res = clamp(o0), x_start = clamp(x_t - ac pred_res - bc o1)
 *                                  3: pred_res = clamp(x_in - o0), x_start = clamp(o0)
 *                             img_out = c1 x_t + c2 pred_res + c3 x_start + exp(logvar / 2) noise, noise(b, t, pixel) the keyed
 *                           stream of seeds[b] above, none at t = 0.  Writes img_out only; img_out == x_t updates in place.
 *                           A mode reads only the streams its formulas name (o0 may be NULL in mode 1, o1 in modes 0 and 3 -- the
 *                           update takes no predicted noise --, x_in in mode 2).  16-byte accesses when npix % 4 == 0 and every
 *                           pointer is 16-byte aligned; the scalar form has the same bits.
 * Both read the step from DEVICE memory: begin -> U-Net forward(s) -> step captures into one HIP graph, G steps at a time.  */
int fd_obj_begin(int *t_dev, const float *times0, const float *times1, float *time0, float *time1, int B, int T,
                 void *stream);
int fd_res_step_obj_keyed(int mode, const float *o0, const float *o1, const float *x_t, const float *x_in,
                          const float *par_table, const int *t_dev, const int64_t *seeds, float *img_out, int B,
                          int64_t npix, int T, void *stream);
/* ---- vanilla DDPM U-Net extras (src/denoising_diffusion_pytorch.py) -----------------------
 * fd_gn_film_silu_apply: silu(GN(h)*(1+scale[b]) + shift[b])   Block w/ scale_shift, 190-199, 213-221
 * fd_chan_ln:            LN over channels * g (+ res)           LayerNorm/PreNorm/Residual, 95-101,127-146
 * fd_linear_attention:   LinearAttention core (227-255) on qkv [B,hw,3*hidden] (to_qkv output):
 *     k softmax over pixels, context = k v^T / hw folded with to_out's weight into
 *     wtot [B][C][hidden] (dtype); q is replaced IN PLACE by softmax_d(q)*scale, so that
 *     to_out(context^T q) is one fd_conv2d over the q slice with per-batch weights.
 *     kstats: fp32 [B][hidden][2], ctx: fp32 [B][hidden/32][32][32] workspaces.
 * fd_attention:          softmax attention, dim_head 32 (257-279): qkv [B,n,3*hidden] -> out [B,n,hidden]
 * fd_lincomb3:           out = ca*a + cb*b + cc*c (b, c may be NULL), optional clamp to [-1,1]:
 *     GaussianDiffusion.predict_* / q_posterior / ddim update (523-554, 633-643)              */
int fd_gn_film_silu_apply(int dtype, const void *h, const float *mean_rstd, const float *gamma,
                          const float *beta, const float *film_scale, const float *film_shift,
                          int film_ld, void *out, int B, int64_t hw, int C, int groups, void *stream);
int fd_chan_ln(int dtype, const void *x, const float *g, const void *res, void *out, int64_t nrows,
               int C, void *stream);
int fd_linear_attention(int dtype, void *qkv, int B, int64_t hw, int hidden, const float *wout,
                        float *kstats, float *ctx, void *wtot, int C, void *stream);
int fd_attention(int dtype, const void *qkv, void *out, int B, int64_t n, int hidden, void *stream);
int fd_lincomb3(const float *a, const float *b, const float *c, float ca, float cb, float cc,
                int clamp, float *out, int64_t n, void *stream);

/* ---- evaluation metrics on device (src/util.py:188-236, used by Trainer.test src/DADiff.py:1883-1885)
 * pred/target [B,H,W] fp32 in [0,1].  partial: fp32 workspace [B][fd_metrics_nblk(H,W)][2].
 * out [B][3] = PSNR (max_val 1), SSIM (11x11 Gaussian sigma 1.5, reflect pad, clamp, mean), RMSE. */
int fd_metrics_nblk(int H, int W);
int fd_metrics(const float *pred, const float *target, int B, int H, int W, float *partial,
               float *out, void *stream);

/* out = a*x + b  (normalize_to_neg_one_to_one / unnormalize, src/DADiff.py:109-120)          */
int fd_affine_f32(const float *x, float a, float b, float *out, int64_t n, void *stream);
/* out = x + s*noise   (x_T = x_input + sqrt(sum_scale) eps, src/DADiff.py:1294)              */
int fd_axpy_f32(const float *x, const float *noise, float s, float *out, int64_t n, void *stream);

/* ---- one training step around the U-Net (fd_train_step.hip; src/DADiff.py:1382-1499, 1689-1725) ---------------
 * fp32, deterministic, no float atomics, no host synchronisation; every summation order depends on the tensor's own
 * size only.  16-byte accesses where the pointers (and npix % 4) allow, the same elements per lane on the scalar path.
 * fd_res_qsample_f32: ResidualDiffusion.forward's normalize (2x - 1, if `normalize`), x_res = x_input - x_start,
 *   q_sample and the cat in one launch.  x_start, x_input, noise [B][npix]; t [B] int64 (clamped to [0, T)); alphas_cumsum,
 *   betas_cumsum [T] on the device.  Give either noise, or seeds [B] int64: then noise = the keyed stream of
 *   fd_keyed_normal(seeds, noise_step) and is written to noise_out.
 *   x_in [B][2][npix] = (x_start + ac x_res + bc noise, x_input), x_res [B][npix], times [2][B] = ac T, bc T.
 * fd_res_loss_f32: loss[0] = scale * mean_b(mean_i(|pred - target| or (pred - target)^2)) (loss_type 1 = l1, 2 = l2) and
 *   dpred = its gradient (sign(0) = 0).  ws: fd_res_loss_ws_floats(B, npix) floats (0: unsupported shape).
 * The optimiser: clip_grad_norm_(max_norm) + torch.optim.Adam (weight_decay 0, no amsgrad) + zero_grad + the EMA update in
 *   three launches over two int64 tables on the device:
 *     chunks  [nchunk][3] = tensor index, offset, length: every tensor cut into fd_opt_chunk_elems() elements from its start
 *     tensors [nt][8]     = p, g, m, v, ema (addresses; ema may be 0), flags (1: has a gradient, 2: all five 16-byte aligned), 0, 0
 *   fd_opt_sumsq_f32     part[chunk] = sum of g^2 (0 without a gradient)
 *   fd_opt_clip_coef     rec[4] = total_norm, coef = min(1, max_norm / (total_norm + 1e-6)) (1 if max_norm < 0), nonfinite, 0;
 *                        steps[i] += 1 for every tensor with a gradient, unless skip_nonfinite and nonfinite
 *   fd_opt_adam_ema_f32  g' = coef g; Adam with the bias corrections of steps[i]; ema_mode 0: none, 1: ema = p,
 *                        2: ema -= (1 - ema_decay)(ema - p); zero_grad: g = 0; writes nothing if skip_nonfinite and nonfinite
 *   fd_opt_radam_ema_f32 the same with torch.optim.RAdam's rule in Adam's place: with s = steps[i], bc1 = 1 - beta1^s,
 *                        bc2 = 1 - beta2^s, rho_inf = 2 / (1 - beta2) - 1 and rho = rho_inf - 2 s beta2^s / bc2, a tensor with
 *                        rho > 5 takes p -= lr / bc1 r sqrt(bc2) m / (sqrt(v) + eps), r = sqrt((rho - 4)(rho - 2) rho_inf /
 *                        ((rho_inf - 4)(rho_inf - 2) rho)), every other one p -= lr / bc1 m; no weight decay */
int fd_res_qsample_f32(const float *x_start, const float *x_input, const int64_t *t, const float *alphas_cumsum,
                       const float *betas_cumsum, int T, const float *noise, const int64_t *seeds, int noise_step,
                       int normalize, float *x_in, float *x_res, float *noise_out, float *times, int B, int64_t npix,
                       void *stream);
int64_t fd_res_loss_ws_floats(int B, int64_t npix);
int fd_res_loss_f32(const float *pred, const float *target, int loss_type, double scale, float *loss, float *dpred,
                    float *ws, int B, int64_t npix, void *stream);
/* out = s_dev[0] * x (the loss gradient times the scalar autograd hands back, read on the device) */
int fd_scale_dev_f32(const float *x, const float *s_dev, float *out, int64_t n, void *stream);
int fd_opt_chunk_elems(void);
int fd_opt_sumsq_f32(const int64_t *chunks, const int64_t *tensors, float *part, int nchunk, void *stream);
int fd_opt_clip_coef(const float *part, int nchunk, const int64_t *tensors, int *steps, int nt, float max_norm,
                     int skip_nonfinite, float *rec, void *stream);
int fd_opt_adam_ema_f32(const int64_t *chunks, const int64_t *tensors, const int *steps, const float *rec, int nchunk,
                        double lr, double beta1, double beta2, double eps, int ema_mode, double ema_decay, int zero_grad,
                        int skip_nonfinite, void *stream);
int fd_opt_radam_ema_f32(const int64_t *chunks, const int64_t *tensors, const int *steps, const float *rec, int nchunk,
                         double lr, double beta1, double beta2, double eps, int ema_mode, double ema_decay, int zero_grad,
                         int skip_nonfinite, void *stream);

/* ---- the gradient sum of data-parallel training (fd_grad_sum.hip; diffusion_train.GradReducer) -----------------
 * fp32, the same in both builds of the library.  Deterministic: plain adds in rank order, no fmaf, no atomics.  Both work over the
 * optimiser's tables above (chunks, tensors) and offs [nt] int64: tensor i lives at [offs[i], offs[i] + numel_i) of a flat buffer,
 * offs = cumsum(numel rounded up to 4), P their total; a flat buffer has N = P + fd_grads_tail_floats() floats, the tail behind the
 * gradients.  Flat buffers are 16-byte aligned; the gradient side takes 16-byte accesses where the tensor's flag allows.
 * fd_grads_pack_f32: flat[offs[i] + k] = g_i[k] (zeros for a tensor without a gradient, zeros in the padding), flat[P + e] =
 *   tail[e] for e < ntail and 0 behind; with `zero`, every g read is then set to 0.
 * fd_grads_rank_sum_f32: recv [W][N], acc [N]; per element v = first ? 0 : acc[i], then v = v + recv[r][i] for r = 0 .. W - 1 in
 *   that order (W <= 64).  If `last`, v goes to the gradient of every tensor that has one (the others are not touched), otherwise
 *   to acc.  The tail's sum always goes to acc[P ..]. */
int fd_grads_tail_floats(void);
int fd_grads_pack_f32(const int64_t *chunks, const int64_t *tensors, const int64_t *offs, int nchunk, float *flat, int64_t P,
                      const float *tail, int ntail, int zero, void *stream);
int fd_grads_rank_sum_f32(const int64_t *chunks, const int64_t *tensors, const int64_t *offs, int nchunk, const float *recv, int W,
                          int64_t N, float *acc, int64_t P, int first, int last, void *stream);

/* ---- what a held-out evaluation reads off a model output (fd_validate.hip) -------------------------------------
 * fd_val_items_f32: items [B][2], from one pass over pred, target (and x_input, x_start) [B][npix] and two small sums, without
 *   a gradient.  items[b][0] = mean_i(|pred - target| or (pred - target)^2) (loss_type 1 = l1, 2 = l2): its mean over b is the
 *   loss of fd_res_loss_f32.  items[b][1] = mean_i((u(x0_hat) - u(x_start))^2), x0_hat = clamp(x_input - clamp(pred, -1, 1), -1, 1)
 *   (the samplers' last step, applied to a residual output), u(v) = clamp((v + 1) / 2, 0, 1): the one-step denoising error in
 *   the [0, 1] units of fd_metrics.  x_input and x_start: both, or both null (column 1 is then NaN).  Deterministic, no float
 *   atomics; a slice's row depends on npix alone, not on its batch.  The shape limits are fd_res_loss_f32's.
 *   ws: fd_val_items_ws_floats(B, npix) floats (0: unsupported shape). */
int64_t fd_val_items_ws_floats(int B, int64_t npix);
int fd_val_items_f32(const float *pred, const float *target, const float *x_input, const float *x_start, int loss_type,
                     float *items, float *ws, int B, int64_t npix, void *stream);

/* ---- the structural term of the training loss (fd_ssim_train.hip; diffusion_train.structural_loss) ------------
 * fp32, the same in both builds of the library.  Deterministic, no atomics; a slice's numbers do not depend on its batch.
 * With y = (x_start + 1) / 2 and p = (x_input - out + 1) / 2 (`residual`) or (out + 1) / 2 (an x0 output), nothing clamped, and
 * w* the window of fd_metrics (11-tap Gaussian, sigma 1.5, normalised, separable, reflect padding of 5), C1 = 0.01^2, C2 = 0.03^2:
 *   mp = w*p, my = w*y, vp = w*p^2 - mp^2, vy = w*y^2 - my^2, c = w*(p y) - mp my
 *   a1 = 2 mp my + C1, a2 = 2 c + C2, b1 = mp^2 + my^2 + C1, b2 = vp + vy + C2, S = a1 a2 / (b1 b2)      (NOT clamped to [0, 1])
 *   items[b] = mean_i S;  term = (float)(scale (1 - mean_b items[b])), the mean in double over the fp32 items
 *   dS/dmu = 2 my a2 / (b1 b2) - S 2 mp / b1, dS/dv = -S / b2, dS/dc = 2 a1 / (b1 b2), A = dS/dmu - 2 mp dS/dv - my dS/dc
 *   d term / d p = -scale (W^T A + 2 p W^T dS/dv + y W^T dS/dc) / N, N = B H W, W^T the adjoint of the reflect-padded filter;
 *   d term / d out = -1/2 of it (`residual`) or +1/2 of it, rounded to fp32
 * fd_ssim_loss_f32: out, x_start [B][H][W]; x_input: slice b at x_input + b x_input_bstride (null and 0 without `residual`).
 *   loss (may be null): loss[0] = term, or loss[0] + term with `accumulate` (one fp32 add).  items (may be null): [B].
 *   dout (may be null: no backward pass runs) [B][H][W] = the gradient, or dout + it with `accumulate` (one fp32 add, no fma).
 *   ws: fd_ssim_loss_ws_floats(B, H, W) floats (0: unsupported shape).  Errors before anything launches: H or W < 6, B > 65535.
 * fd_onestep_u01_f32: est = u(clamp(x_input - clamp(pred, -1, 1), -1, 1)), tgt = u(x_start), u(v) = clamp((v + 1) / 2, 0, 1),
 *   all [B][npix] (x_input strided as above): the one-step estimate of fd_val_items_f32 as the image pair fd_metrics reads. */
int64_t fd_ssim_loss_ws_floats(int B, int H, int W);
int fd_ssim_loss_f32(const float *out, const float *x_input, int64_t x_input_bstride, const float *x_start, int residual,
                     double scale, float *loss, float *items, float *dout, int accumulate, float *ws, int B, int H, int W,
                     void *stream);
int fd_onestep_u01_f32(const float *pred, const float *x_input, int64_t x_input_bstride, const float *x_start, float *est,
                       float *tgt, int B, int64_t npix, void *stream);

/* ---- an ensemble of K keyed realisations per slice (fd_ensemble.hip; ResidualDiffusion.sample_ensemble) --------
 * fp32, the same in both builds of the library.  Deterministic, no float atomics.
 * fd_rows_repeat_f32: dst [B K][n], dst[b K + k] = src[b] (src [B][n]): a slice's input plane or conditioning row, once per
 *   replica.  16-byte accesses when n % 4 == 0 and both pointers are 16-byte aligned, scalar otherwise.
 * fd_ensemble_stats_f32: samples [B][K][n] -> mean [B][n] = (the fp32 sum in k order) / K; std [B][n] = the two-pass sample
 *   standard deviation sqrt(sum_k (x - mean)^2 / (K - 1)) in k order, exactly 0 for K = 1; spread [B] = sqrt(mean_i std^2).
 *   A slice's rows depend on K and n alone, not on B or on the other slices; the 16-byte form (n % 4 == 0, samples, mean and
 *   std 16-byte aligned) and the scalar form give the same bits.  ws: B * fd_ensemble_nblk(n) floats (0: unsupported n). */
int fd_ensemble_nblk(int64_t n);
int fd_rows_repeat_f32(const float *src, float *dst, int B, int K, int64_t n, void *stream);
int fd_ensemble_stats_f32(const float *samples, float *mean, float *std, float *ws, float *spread, int B, int K, int64_t n,
                          void *stream);

/* ---- per-pixel order statistics of an ensemble and the coverage of a target (fd_ensemble_order.hip;
 * ResidualDiffusion.sample_ensemble(quantiles=...), metrics.ensemble_quantiles, metrics.interval_coverage) --------
 * fp32, the same in both builds of the library.  Deterministic, no float atomics.
 * fd_ensemble_order_f32: samples [B][K][n] -> out [B][Q][n].  Per pixel, with its K values in ascending order v_(0) <= ... <=
 *   v_(K-1): out[b][j] = fmaf(frac[j], v_(hi[j]) - v_(lo[j]), v_(lo[j])), and v_(lo[j]) itself, bit for bit, where frac[j] == 0
 *   (minimum, maximum, the median of an odd K, every level at K = 1).  lo, hi (int) and frac (float) are HOST arrays of Q entries,
 *   read in the entry and handed to the kernel by value: no device table, no upload, and the call can be captured.
 *   1 <= Q <= 8, 0 <= lo <= hi <= K - 1, 0 <= frac <= 1, 1 <= K <= 65535, 1 <= B <= 65535, 0 < n < 2^40.  Equal values are
 *   interchangeable (a pixel that holds -0 and +0 may return either).  If any of a pixel's K values is NaN, every level of that
 *   pixel is NaN.  K <= 32 sorts in registers (every sample read once); a larger K selects by counting ranks and reads the K values
 *   K / 4 times, so its time grows with K^2.  Both give the same bits, and so do the 16-byte form (n % 4 == 0, samples and out
 *   16-byte aligned) and the scalar form.  A pixel's outputs depend on its own K values and the table alone, not on B, the other
 *   slices or the launch.  No workspace.
 * fd_ensemble_coverage_f32: count [B] (int64) = the number of pixels i < n with lo_map[b][i] <= target[b][i] <= hi_map[b][i]; a
 *   NaN compares false.  Slice b of each map starts b * its own stride (in floats, >= 0) past the pointer, so the two maps may be
 *   rows of one out [B][Q][n] (stride Q n).  Exact: integer block counts, added per slice in index order.  16-byte accesses when
 *   n % 4 == 0, the three pointers are 16-byte aligned and the strides are multiples of 4; scalar otherwise.
 *   ws: B * fd_ensemble_coverage_nblk(n) ints (0: unsupported n). */
int fd_ensemble_order_f32(const float *samples, float *out, const int *lo, const int *hi, const float *frac, int B, int K, int Q,
                          int64_t n, void *stream);
int fd_ensemble_coverage_nblk(int64_t n);
int fd_ensemble_coverage_f32(const float *lo_map, int64_t lo_bstride, const float *hi_map, int64_t hi_bstride, const float *target,
                             int64_t target_bstride, int *ws, int64_t *count, int B, int64_t n, void *stream);

/* ---- calibrated ensemble intervals: the scale that makes [centre - scale d_lo, centre + scale d_hi] cover a target (fd_interval.hip;
 * metrics.interval_hist, metrics.interval_scale, Trainer.calibrate_intervals, Trainer.test(interval_scale=...)) --------
 * fp32, the same in both builds of the library.  Deterministic, no float atomics, no atomics on global memory.  Per pixel, with the
 * centre m, the lower map l, the upper map u and floor > 0:  d_lo = fmaxf(m - l, floor),  d_hi = fmaxf(u - m, floor), each
 * difference one fp32 rounding.  Slice b of each input map starts b * its own stride (in floats, >= 0) past the pointer, as in
 * fd_ensemble_coverage_f32, so l and u may be rows of one [B][Q][n] tensor of quantiles.  16-byte accesses when n % 4 == 0, every map
 * pointer is 16-byte aligned and the strides are multiples of 4; scalar otherwise: the same results.  A slice's results do not depend
 * on B or on the other slices.  1 <= B <= 65535, 0 < n < 2^34.
 * fd_interval_hist_f32: hist [B][G + 1] (int64).  The score of a pixel against the target y is
 *   s = fmaxf((m - y) / d_lo, (y - m) / d_hi), each difference and each quotient one correctly rounded fp32 operation: the smallest
 *   scale whose interval holds y.  grid: G ascending floats in DEVICE memory, 1 <= G <= 4096 (the caller vouches for the order).
 *   hist[b][j] = the number of pixels of slice b whose bin is j; the bin is the number of grid values strictly below s, so
 *   s == grid[g] falls in bin g.  A pixel with a NaN among m, l, u, y, or whose either quotient is NaN (inf / inf), is covered at no
 *   scale and goes to bin G, as s = +inf does.  Every row sums to n.  Form: per-workgroup partial histograms in LDS (grid and
 *   counters, 2 x 16 KB; lanes of a wave that share a bin are counted by ballot and added once), written to ws and added per slice
 *   in index order by a second launch.  ws: B * fd_interval_hist_nblk(n) * (G + 1) ints (nblk 0: unsupported n).
 * fd_interval_scale_f32: lo_out, hi_out [B][n] (dense), width [B].  lo_out = min(max(m - scale d_lo, 0), 1) and
 *   hi_out = min(max(m + scale d_hi, 0), 1), the product and the sum two separate fp32 roundings; scale >= 0.  width[b] = the mean
 *   over the slice's pixels of hi_out - lo_out: fp32 workgroup sums, added per slice in index order in double.  A NaN in m, l or u
 *   makes lo_out and hi_out NaN at that pixel and at no other, and makes width[b] NaN: the mean is not taken over the rest.
 *   ws: B * fd_interval_scale_nblk(n) floats (0: unsupported n). */
int fd_interval_hist_nblk(int64_t n);
int fd_interval_hist_f32(const float *center, int64_t center_bstride, const float *lo_map, int64_t lo_bstride, const float *hi_map,
                         int64_t hi_bstride, const float *target, int64_t target_bstride, const float *grid, int G, float floor,
                         int *ws, int64_t *hist, int B, int64_t n, void *stream);
int fd_interval_scale_nblk(int64_t n);
int fd_interval_scale_f32(const float *center, int64_t center_bstride, const float *lo_map, int64_t lo_bstride, const float *hi_map,
                          int64_t hi_bstride, float scale, float floor, float *lo_out, float *hi_out, float *ws, float *width, int B,
                          int64_t n, void *stream);

/* ---- an ensemble over the orientations of the square (fd_ensemble_orient.hip; ResidualDiffusion.sample_ensemble(orientations=...),
 * founddiff_amd/ensemble.py) --------
 * fp32, the same in both builds of the library.  Deterministic, no float atomics.  A code is the training augmentation's (the slice
 * store below): bit 0 flips H, bit 1 flips W, bits 2-3 = k, out = rot90(flip_W(flip_H(m)), k); codes are DEVICE int32 arrays of K
 * entries, one per replica.  1 <= B, K <= 65535, H, W <= 32768.
 * fd_rows_orient_f32: src [B][H W] -> dst [B K][H W], dst[b K + k] = src[b] under codes[k]: a copy, the repeat of
 *   fd_rows_repeat_f32 and the orientation in one launch.  The entry reads the K codes back (it waits for the stream): a code
 *   outside 0..15, or a transposing code (bit 2) with H != W, returns an error and nothing is launched.  16-byte accesses (reversed in
 *   registers under a W flip, through a padded LDS tile where the code transposes) when W % 4 == 0 and both pointers are 16-byte
 *   aligned; scalar otherwise: the same bits.
 * fd_ensemble_orient_stats_f32: samples [B][K][H W], replica k in its own orientation -> mean, std [B][H W], spread [B] and, where
 *   samples_out ([B K][H W]) is not NULL, the K un-oriented images; replica k's pixel is read through inv_codes[k], the code of the
 *   INVERSE of its orientation (ensemble.orientation_inverse; the low 4 bits are used, and a transposing code on H != W is read as
 *   its non-transposing part: no argument reads outside samples).  All outputs have the bits of un-orienting every replica followed
 *   by fd_ensemble_stats_f32(B, K, H W); mean, std and spread are the same with and without samples_out.  A slice's rows depend on K,
 *   H, W, the codes and its own samples alone.  Between its two launches std holds the variance.  16-byte accesses when W % 4 == 0
 *   and samples, mean, std (and samples_out, if given) are 16-byte aligned; the scalar form has the same bits.
 *   ws: B * fd_ensemble_nblk(H W) floats.
 * fd_rows_take_f32: dst [R][n], dst[r] = src[idx[r]] (idx DEVICE int32 [R], every entry a row of src): conditioning rows shared by
 *   the replicas of one orientation.  fd_rows_repeat_f32's alignment rule. */
int fd_rows_orient_f32(const float *src, float *dst, const int *codes, int B, int K, int H, int W, void *stream);
int fd_ensemble_orient_stats_f32(const float *samples, const int *inv_codes, float *mean, float *std, float *ws, float *spread,
                                 float *samples_out, int B, int K, int H, int W, void *stream);
int fd_rows_take_f32(const float *src, float *dst, const int *idx, int R, int64_t n, void *stream);

/* ---- a slice as overlapping tiles (fd_tiles.hip; ResidualDiffusion.sample_tiled; founddiff_amd/tiling.py) --------
 * fp32, the same in both builds of the library.  Deterministic, no atomics, no workspace.  The plan: my x mx tiles of th x tw
 * pixels at the origins ys [my], xs [mx] (int32, DEVICE memory; 0 <= ys <= H - th, 0 <= xs <= W - tw, a tile whose origin is
 * outside that range is not touched); tile row r = (b my + iy) mx + ix.  xs_mult4: the host's word that every xs is a multiple
 * of 4.  1 <= th <= H, 1 <= tw <= W, my, mx >= 1, B my mx <= 65535, H, W <= 32768.
 * fd_tiles_gather_f32: dst [B my mx][th tw], dst[r] = the window of src[b] ([B][H W]) at (ys[iy], xs[ix]): a copy.  16-byte
 *   accesses when xs_mult4, W % 4 == 0, tw % 4 == 0 and src, dst are 16-byte aligned, scalar otherwise: the same bits.
 * fd_tiles_blend_f32: out [B][H W]; per pixel, over the tiles that cover it in row-major tile order (iy, then ix ascending):
 *   w = wy[iy][y - ys[iy]] * wx[ix][x - xs[ix]] (wy [my][th], wx [mx][tw]), num = fmaf(w, v, num), den += w, out = num / den
 *   with the correctly rounded division.  A gather: one lane per 4 pixels of an output row, so a pixel depends on H, W, the plan
 *   and its covering tiles alone, not on B.  A pixel under ONE tile whose weight there is 1 (tiling.tile_weights gives that) has
 *   den = 1 and out = that tile's value, bit for bit.  The 16-byte form (xs_mult4, W % 4 == 0, tw % 4 == 0, tiles, wx and out
 *   16-byte aligned) and the scalar form give the same bits.  A pixel no tile covers is 0 / 0. */
int fd_tiles_gather_f32(const float *src, float *dst, const int *ys, const int *xs, int B, int H, int W, int th, int tw, int my,
                        int mx, int xs_mult4, void *stream);
int fd_tiles_blend_f32(const float *tiles, const float *wy, const float *wx, const int *ys, const int *xs, float *out, int B,
                       int H, int W, int th, int tw, int my, int mx, int xs_mult4, void *stream);
/* ---- one sampler step of a slice held as tiles, the tiles' model outputs blended per pixel first (fd_tiles_step.hip;
 * ResidualDiffusion.sample_tiled(fuse="step")).  fp32, the same in both builds; no atomics, no workspace.  The plan and weight
 * arguments and the shape limits are fd_tiles_blend_f32's; o0, o1, x_t, x_in, img_out are [B my mx][th tw] in tile-row order.  A
 * lane owns 4 consecutive pixels of one tile row and, for its pixel (y, x) of slice b,
 *   blends  each stream the mode reads over the covering tiles in row-major tile order with fd_tiles_blend_f32's arithmetic
 *           (modes 0 and 3 read o0, mode 1 o1, mode 2 both; x_in may be NULL in mode 2),
 *   updates with the blended outputs, its own x_t and its own x_in:
 *           fd_tiles_step_ddim_f32   fd_res_step_obj's step 1 without noise; par (DEVICE, 8 floats, shared by all rows) =
 *                                    {ac, bc, omac, alpha, -, -, -, last}: last != 0 ? x_start : x_t - alpha pred_res
 *           fd_tiles_step_keyed_f32  fd_res_step_obj_keyed's update, row t = *t_dev (held in [0, T)) of par_table [T][8]; the noise
 *                                    is that of the SLICE pixel, element (y W + x) % 4 of the keyed stream's group (y W + x) / 4
 *                                    under slice_seeds[b] ([B]: one seed per slice) -- fd_keyed_normal's field over the slice --
 *                                    so overlapping tiles receive the same noise; none at t = 0,
 *   writes  img_out (which may be x_t: a lane reads other tiles' o0 / o1 only) and, where slice_out ([B][H W], may be NULL) is
 *           given and its tile is the first of the covering tiles in that order, the slice pixel.
 * Rows gathered from slice-level x_t and x_in (fd_tiles_gather_f32) leave the step with equal bits in the common pixels of
 * overlapping tiles; a one-tile plan has the bits of fd_res_step_obj / fd_res_step_obj_keyed.  16-byte accesses when xs_mult4,
 * W % 4 == 0, tw % 4 == 0 and every pointer in use is 16-byte aligned; the scalar form has the same bits. */
int fd_tiles_step_ddim_f32(int mode, const float *o0, const float *o1, const float *x_t, const float *x_in, const float *par,
                           const float *wy, const float *wx, const int *ys, const int *xs, int B, int H, int W, int th, int tw,
                           int my, int mx, int xs_mult4, float *img_out, float *slice_out, void *stream);
int fd_tiles_step_keyed_f32(int mode, const float *o0, const float *o1, const float *x_t, const float *x_in,
                            const float *par_table, const int *t_dev, const int64_t *slice_seeds, const float *wy, const float *wx,
                            const int *ys, const int *xs, int B, int H, int W, int th, int tw, int my, int mx, int xs_mult4,
                            float *img_out, float *slice_out, int T, void *stream);
/* ---- the final tile images of K keyed realisations per slice, to the ensemble's statistics (fd_tiles_ensemble.hip;
 * ResidualDiffusion.sample_ensemble(tile=...)).  fp32, the same in both builds; no atomics.  tiles [B K my mx][th tw], row
 * ((b K + k) my + iy) mx + ix; the plan and weight arguments are fd_tiles_blend_f32's, the limit is B K my mx <= 65535, K >= 1.
 * mean, std [B][H W], spread [B], ws: B * fd_ensemble_nblk(H W) floats; samples [B K][H W], or NULL: the K blended slice images
 * are then not written (mean, std and spread are the same).  All four outputs have the bits of fd_tiles_blend_f32 over the B K
 * pseudo-slices followed by fd_ensemble_stats_f32(B, K, H W): a slice's rows depend on K, H, W, the plan and its own tiles alone.
 * 16-byte accesses when xs_mult4, W % 4 == 0, tw % 4 == 0 and tiles, wx, mean, std (and samples, if given) are 16-byte aligned;
 * the scalar form has the same bits. */
int fd_tiles_ensemble_f32(const float *tiles, const float *wy, const float *wx, const int *ys, const int *xs, float *samples,
                          float *mean, float *std, float *ws, float *spread, int B, int K, int H, int W, int th, int tw, int my,
                          int mx, int xs_mult4, void *stream);

/* ---- a training batch from a slice store on the device (fd_train_data.hip; data/pdf_dataset.py:521-545) -------
 * nd [n_nd][H][W], ld [n_ld][H][W] fp32 in [0, 1].  Item b of the batch is the pair nd[nd_slot[b]], ld[ld_slot[b]] (int64 [B],
 * clamped to the store), both under the transform codes[b] (int64 [B], low 4 bits; a null codes is all 0):
 *   bit 0 flips H, bit 1 flips W, bits 2-3 = k: out = rot90(flip_W(flip_H(m)), k).  Source pixel (i, j) of output pixel (y, x):
 *   k = 0 (y, x), 1 (x, W-1-y), 2 (H-1-y, W-1-x), 3 (H-1-x, y); then j = W-1-j if bit 1 and i = H-1-i if bit 0.  An odd k needs
 *   H == W (it is dropped otherwise).  Even k: every lane owns 4 consecutive output pixels and reads 4 consecutive source
 *   pixels; odd k: a workgroup owns a 64 x 64 output tile and turns it in the LDS (per pixel where W % 4 != 0 or a pointer
 *   is not 16-byte aligned).  The form is chosen per slice.  B <= 65535, H, W <= 32768; no atomics, no host synchronisation.
 * fd_store_gather_f32: x_start, x_input [B][H][W] = the two transformed images: a copy.
 * fd_res_qsample_store_f32: fd_res_qsample_f32 on that batch without assembling it: the same arithmetic, and output pixel p
 *   (row-major in the output) takes element p % 4 of the keyed stream's group p / 4, so every output has the bits of
 *   fd_store_gather_f32 followed by fd_res_qsample_f32.  noise [B][H][W] is in output order.  x0 (nullable) [B][H][W] = the
 *   normalised x_start (the target of pred_x0_noise). */
int fd_store_gather_f32(const float *nd, const float *ld, int64_t n_nd, int64_t n_ld, const int64_t *nd_slot,
                        const int64_t *ld_slot, const int64_t *codes, float *x_start, float *x_input, int B, int H, int W,
                        void *stream);
int fd_res_qsample_store_f32(const float *nd, const float *ld, int64_t n_nd, int64_t n_ld, const int64_t *nd_slot,
                             const int64_t *ld_slot, const int64_t *codes, const int64_t *t, const float *alphas_cumsum,
                             const float *betas_cumsum, int T, const float *noise, const int64_t *seeds, int noise_step,
                             int normalize, float *x_in, float *x_res, float *noise_out, float *times, float *x0, int B,
                             int H, int W, void *stream);

/* ---- the same batch cut to patches (fd_train_crop.hip; CropToFixed, data/transforms.py:196-249) --------------
 * As above, with windows (int64 [B][2] = y0, x0 per item; null: all 0) and the crop CH x CW: item b is first cut to the window
 * [y0, y0 + CH) x [x0, x0 + CW) of its slices (y0, x0 clamped to [0, max(H - CH, 0)] x [0, max(W - CW, 0)]); an axis no longer
 * than the crop is taken whole and reflect-padded to it, (c - n) / 2 in front and the rest behind, without an edge repeat and
 * with one reflection: a pad of at most H - 1 / W - 1 on either side.  The code then applies to the crop: source pixel
 * (refl(y0 - pad_top + ic, H), refl(x0 - pad_left + jc, W)) for the crop pixel (ic, jc) the map above gives on CH x CW;
 * refl(v, n) = -v below 0, 2 (n - 1) - v from n on.  An odd k needs CH == CW (it is dropped otherwise), whatever H and W are.
 * Every output is [B][CH][CW]; the forms are those above on CH, CW (per pixel where CW % 4 != 0 or an output pointer is not
 * 16-byte aligned).  The source rows are read at 4-byte alignment, so nd and ld need none.  H, W, CH, CW <= 32768.
 * fd_store_crop_f32: x_start, x_input = the two cropped, transformed images: a copy.
 * fd_res_qsample_crop_f32: fd_res_qsample_f32 on that batch without assembling it; output pixel p of the crop takes element
 *   p % 4 of the keyed stream's group p / 4: the bits of fd_store_crop_f32 followed by fd_res_qsample_f32. */
int fd_store_crop_f32(const float *nd, const float *ld, int64_t n_nd, int64_t n_ld, const int64_t *nd_slot,
                      const int64_t *ld_slot, const int64_t *codes, const int64_t *windows, float *x_start, float *x_input,
                      int B, int H, int W, int CH, int CW, void *stream);
int fd_res_qsample_crop_f32(const float *nd, const float *ld, int64_t n_nd, int64_t n_ld, const int64_t *nd_slot,
                            const int64_t *ld_slot, const int64_t *codes, const int64_t *windows, const int64_t *t,
                            const float *alphas_cumsum, const float *betas_cumsum, int T, const float *noise,
                            const int64_t *seeds, int noise_step, int normalize, float *x_in, float *x_res, float *noise_out,
                            float *times, float *x0, int B, int H, int W, int CH, int CW, void *stream);

/* ---- the two outer convolutions of the U-Net for training (fd_outer_train.hip; src/DADiff.py:553-555, 681) ----
 * Exact fp32 on the VALU, deterministic, no float atomics, no host synchronisation; out and dx of a slice do not depend on its
 * batch.  Byte bounds: DESIGN.md section 4.
 * fd_init_conv7_fwd_f32: x [B][Cin][H][W] planes (Cin 2 or 3), weight [Cout][Cin][7][7], bias [Cout] -> out [B][H][W][Cout],
 *   padding 3.  Cout a multiple of 32, at most 512.
 * fd_init_conv7_wgrad_f32: g [49 Cin + 1][Cout]: g[(c 7 + kh) 7 + kw][co] = dweight[co][c][kh][kw], the last row dbias; one pass
 *   over dout [B][H][W][Cout] (tiles of it and their halo of x in the LDS), split over at most 1024 ranges of tiles whose
 *   partials two more launches add in order.  ws: fd_init_conv7_wgrad_ws_floats(...) floats (0: unsupported shape).
 * fd_final_conv1_fwd_f32: out[p] = bias[0] + sum_c x[p][off + c] weight[c], x rows ld floats apart (a channel slice is read in
 *   place; x points at the row start, ld and off multiples of 4).  C a multiple of 4, at most 1024; npix <= 2^30.
 * fd_final_conv1_bwd_f32: dx [npix][C] = dout[p] weight[c]; dwb [C + 4] = dweight, dbias, 0, 0, 0; reads x and dout once.
 *   ws: fd_final_conv1_bwd_ws_floats(npix, C) floats (0: unsupported shape). */
int fd_init_conv7_fwd_f32(const float *x, const float *weight, const float *bias, float *out, int B, int Cin, int H, int W,
                          int Cout, void *stream);
int64_t fd_init_conv7_wgrad_ws_floats(int B, int Cin, int H, int W, int Cout);
int fd_init_conv7_wgrad_f32(const float *x, const float *dout, float *g, float *ws, int B, int Cin, int H, int W, int Cout,
                            void *stream);
int fd_final_conv1_fwd_f32(const float *x, int ld, int off, const float *weight, const float *bias, float *out, int64_t npix,
                           int C, void *stream);
int64_t fd_final_conv1_bwd_ws_floats(int64_t npix, int C);
int fd_final_conv1_bwd_f32(const float *x, int ld, int off, const float *weight, const float *dout, float *dx, float *dwb,
                           float *ws, int64_t npix, int C, void *stream);

#ifdef __cplusplus
}
#endif
#endif
