// fd_scan.hip -- SS2D selective scan for gfx950: chunked 3-phase parallel prefix over the
// sequence, fp32 state, one lane per channel (coalesced NHWC loads), the per-position
// (dt_r, B, C) row wave-uniform (scalar loads).
//
//   phase A  (parallel over chunks)  local scan from h=0:  H_c[n] and sum of dt -> P_c[n]=exp(A[n]*sum dt)
//   phase B  (parallel over segments of chunks) carry-in of every chunk: h_in[c+1] = P_c h_in[c] + H_c
//   phase C  (parallel over chunks)  re-run the recurrence from h_in, y = sum_n h C + D u
//
// The EfficientScan gather (4 stride-2 sub-grids, two of them column-major) and the
// EfficientMerge scatter are index arithmetic on the NHWC tensors: neither the (B,4,D,L)
// gathered tensor, nor delta (dt_proj + bias + softplus is recomputed per step from the
// R-vector), nor dA/dBu ever exist in HBM.  Algorithmic HBM bytes per (pixel, channel):
// u read twice + y written once (dtype), plus the x_dbl rows (fp32, shared by all channels).
#include "fd_common.h"
#include <stdlib.h>

namespace {

struct ScanGeom {
    int B, H, W, D, N, R, CD;
    int H2, W2, L, CL, nch;
    const void *xw;      // bf16 x_proj weights [4][CD][D], or NULL: phase A computes the chunk's x_dbl rows itself
    float *xdbl_out;     // ... and writes them here for phase C
    bool low_latency;    // FD_OPT_LOW_LATENCY: chunked scan at every size (include/founddiff_hip.h)
};

// position l of direction k -> (row of xdbl, NHWC pixel index inside the image)
__device__ __forceinline__ void scan_pos(const ScanGeom &g, int k, int l, int &lrow, int &pix) {
    int h2, w2;
    if (k & 1) { w2 = l / g.H2; h2 = l - w2 * g.H2; }
    else { h2 = l / g.W2; w2 = l - h2 * g.W2; }
    lrow = h2 * g.W2 + w2;
    pix = (2 * h2 + (k & 1)) * g.W + 2 * w2 + (k >> 1);
}

// One workgroup = one chunk of one (batch, direction) x up to 4 waves of 64 channels.  The
// chunk's x_dbl rows (dt_r | B | C, shared by every channel) are staged once in LDS and read
// back as wave-uniform broadcasts; each lane prefetches U of its u values per group so U
// global loads are in flight per wave while the recurrence of the previous group runs.
// ODD: H or W is odd.  The reference pads the image to even sizes with zeros before the gather and crops after the
// merge (src/emamba2.py:191-199, 253-260): the padded positions take part in the recurrence with u = 0 and a zero
// x_dbl row (x_proj has no bias), i.e. the state only decays by exp(softplus(dt_bias) A) there, and their outputs
// are dropped.  Here they are positions whose pixel lies outside the image: u := 0, no store; the x_dbl rows of
// those positions are zeros written by the x_proj launch (its gather zero-fills out-of-range pixels).
// CPL = channels per lane.  2 (bf16, N <= 8: the 512x512 / 256x256 levels, where these kernels are bound by VALU
// issue, PMC 73-95 % busy): a lane owns two NEIGHBOURING channels and every float pair is (channel, channel + 1)
// instead of (state, state + 1) -- the dt_proj contraction, dt*u, the D skip and the y accumulator become packed
// instructions too, the cross-half add of the y pair disappears, u / y move as one dword per lane and step, and a
// wave's LDS row broadcasts serve 128 channels: ~26.5 instead of ~31 issue slots per (channel, position).
template <typename T, int N, int R, bool FINAL, bool ODD, int CPL = 1>
// (occupancy steps: N = 16 with dt_rank >= 16 wants 100-114 registers -- at 5 waves per SIMD it spilled 16-20 bytes: 4 waves measured
//  418-427 -> 406-412 us for d_inner 512 at 128x128; with dt_rank 8 the 5-wave form is the faster one, 202 vs 212 us)
__global__ __launch_bounds__(256, (N >= 32 ? 3 : (N >= 16 && R >= 16 ? 4 : (N >= 8 ? (CPL == 2 ? 4 : 5) : 1)))) void scan_chunk_kernel(const T *__restrict__ xc, const float *__restrict__ xdbl,
                                                        const float *__restrict__ dtw, const float *__restrict__ dtb,
                                                        const float *__restrict__ A, const float *__restrict__ Ds,
                                                        T *__restrict__ y, float *__restrict__ wsH,
                                                        float *__restrict__ wsP, const ScanGeom g) {
    constexpr int CD = R + 2 * N;
    constexpr int CDP = (CD + 3) & ~3;
    // bf16 mode: dt is carried as L = log2(1 + 2^z), z = log2e*(w.x + bias), i.e. dt/ln2.  log2e is folded
    // into w and bias, exp(dt*A) = exp2(L*A) needs no constant at all, and the state is h/ln2 in both
    // passes and in the carries (linear in dt*u) -- softplus shrinks from 7 VALU instructions to 4
    // (v_min, v_exp, v_add, v_log).  z is clamped at 126: 1 + 2^z == 2^z there, so L == z exactly.
    constexpr bool LOG2U = sizeof(T) == 2;
    constexpr float WS = LOG2U ? 1.4426950408889634f : 1.f;          // scale of w, bias
    constexpr float AS = LOG2U ? 1.f : 1.4426950408889634f;          // scale of A
    extern __shared__ __attribute__((aligned(16))) float sx[];      // [CL][CDP]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nw = blockDim.x >> 6;
    static_assert(CPL == 1 || (CPL == 2 && sizeof(T) == 2), "two channels per lane: bf16 only");
    const int dgroups = g.D / (64 * CPL * nw);
    const int chunk = blockIdx.x / dgroups, dg = blockIdx.x - chunk * dgroups;
    const int bk = blockIdx.y, b = bk >> 2, k = bk & 3;
    const int d = ((dg * nw + wave) * 64 + lane) * CPL;
    const int kd = k * g.D + d;
    const int l0 = chunk * g.CL;
    const int l1 = min(l0 + g.CL, g.L);
    const int odd = k & 1, ph = k & 1, pw = k >> 1;
    const float *xb = xdbl + ((int64_t)k * g.B + b) * g.L * g.CD;   // [4][B][L][CD]

    // ---- fused x_proj (phase A, bf16, one workgroup per chunk): x_dbl[l][e] = sum_c Wx[k][e][c] xc[pix(l)][c]
    // (src/emamba2.py:332 einsum) on the matrix cores, straight into the LDS row buffer and out to the x_dbl
    // workspace phase C stages from.  The separate x_proj launch read the whole xc tensor once more from HBM
    // (0.17 ms per batch-8 launch at 512x512); here that read is the first touch of the chunk's pixels and the
    // recurrence's own u loads below hit L2.  Transposed issue: rows = outputs e, columns = 16 positions.
    // (Round 4, measured: they do NOT hit -- FETCH_SIZE of this phase is 2x u.  tools/probes/fetch_calib.hip: a streaming
    // kernel turns an XCD's 4 MB L2 over in ~3 us (a re-touch 3 us after the first touch goes back to memory 74 % of
    // the time, an immediate one never), and the recurrence re-touches a chunk's pixels up to 128 steps later.  Two
    // interleaved forms were built -- x_proj block by block in front of its 16 recurrence steps, fragment and u loads
    // one group apart (fetch +14 %, time equal) or issued together (the extra live registers spill at 4 waves per
    // SIMD: 2x slower) -- and dropped; the kernel is VALU-bound and the second read costs bytes, not time.)
    if constexpr (!FINAL && sizeof(T) == 2 && CPL != 2) {
        if (g.xw) {
            const bf16 *Wk = (const bf16 *)g.xw + (int64_t)k * CD * g.D;
            const bf16 *ubx = (const bf16 *)xc + (int64_t)b * g.H * g.W * g.D;
            float *xo = g.xdbl_out + ((int64_t)k * g.B + b) * g.L * g.CD;
            constexpr int MB = (CD + 15) / 16;
            const int fr = lane & 15, fg = lane >> 4;
            const int nblk = (l1 - l0 + 15) >> 4;
            // Every pixel load of a 16-position block is in flight before its first MFMA, and the NEXT block's loads
            // are issued in front of the current block's MFMAs.  (With the K loop's trip count a runtime value the loop
            // was not unrolled and each K32 step waited for its own pixel load: a chain of d_inner / 32 HBM round trips
            // per block, 32 of them per workgroup at level 0 -- several times the 128 steps of recurrence that follow;
            // PMC of phase A: VALU 64 % busy, 53 % of wave time parked, against 87 % / 36 % in phase C.)
            constexpr int KSM = CPL == 2 ? 4 : 8;                   // K32 steps: d_inner <= 128 (CPL == 2, launcher) / <= 256
            const int nks = g.D >> 5;
            struct BlkPos { int l, lrow; };
            auto fetch = [&](int nb, BlkPos &q, bf16x8 (&bq)[KSM]) {
                const int l = l0 + nb * 16 + fr;
                int h2, w2;
                if (odd) { w2 = l / g.H2; h2 = l - w2 * g.H2; }
                else { h2 = l / g.W2; w2 = l - h2 * g.W2; }
                const int hh = 2 * h2 + ph, ww = 2 * w2 + pw;
                const bool inimg = l < l1 && hh < g.H && ww < g.W;      // odd sizes: padded positions are zero rows
                const bf16 *px = ubx + ((int64_t)hh * g.W + ww) * g.D + 8 * fg;
                q.l = l;
                q.lrow = h2 * g.W2 + w2;
#pragma unroll
                for (int ks = 0; ks < KSM; ++ks) {
                    bq[ks] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
                    if (ks < nks && inimg) bq[ks] = *(const bf16x8 *)(px + 32 * ks);
                }
            };
            // (the second register set only where it is free: 16 registers at d_inner = 128; at 256 the N >= 8 kernels
            // sit at their 96-register occupancy step and the workgroup's waves share the blocks anyway)
            constexpr bool DB = KSM == 4;
            BlkPos cur, nxt;
            bf16x8 bcur[KSM], bnxt[DB ? KSM : 1];
            if (DB && wave < nblk) fetch(wave, cur, bcur);
            for (int nb = wave; nb < nblk; nb += nw) {
                const bool more = DB && nb + nw < nblk;
                if constexpr (DB) { if (more) fetch(nb + nw, nxt, bnxt); }
                else fetch(nb, cur, bcur);
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) {
                    const int e = mb * 16 + fr;
                    bf16x8 afr[KSM];
#pragma unroll
                    for (int ks = 0; ks < KSM; ++ks) {
                        afr[ks] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
                        if (ks < nks && e < CD) afr[ks] = *(const bf16x8 *)(Wk + (int64_t)e * g.D + 32 * ks + 8 * fg);
                    }
                    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < KSM; ++ks)
                        if (ks < nks) acc = FD_MFMA16(afr[ks], bcur[ks], acc, 0, 0, 0);
                    const int e0 = mb * 16 + 4 * fg;                    // CD % 4 == 0 (launcher): all four or none
                    if (cur.l < l1 && e0 < CD) {
                        *(f32x4 *)&sx[(nb * 16 + fr) * CDP + e0] = acc;
                        *(f32x4 *)&xo[(int64_t)cur.lrow * CD + e0] = acc;
                    }
                }
                if constexpr (DB) {
                    if (more) {
                        cur = nxt;
#pragma unroll
                        for (int ks = 0; ks < KSM; ++ks) bcur[ks] = bnxt[ks];
                    }
                }
            }
        }
    }
    // ---- the same on fp32 storage (the fp32s engine, FD_OPT_F32_SPLIT): fp32 pixels and fp32 x_proj weights, every product as
    // three bf16 MFMAs on hi / lo operand halves (x_hi.w_hi + x_lo.w_hi + x_hi.w_lo, ~2^-16: the arithmetic of that engine's
    // other contractions).  Round 6: until then the fp32 modes ran x_proj as its own launch (4 stride-2 sub-grid GEMMs over xc).
    if constexpr (!FINAL && sizeof(T) == 4) {
        if (g.xw) {
            const float *Wk = (const float *)g.xw + (int64_t)k * CD * g.D;
            const float *ubx = (const float *)xc + (int64_t)b * g.H * g.W * g.D;
            float *xo = g.xdbl_out + ((int64_t)k * g.B + b) * g.L * g.CD;
            constexpr int MB = (CD + 15) / 16, KSM = 8;               // d_inner <= 256 (launcher)
            const int fr = lane & 15, fg = lane >> 4;
            const int nblk = (l1 - l0 + 15) >> 4;
            const int nks = g.D >> 5;
            for (int nb = wave; nb < nblk; nb += nw) {
                const int l = l0 + nb * 16 + fr;
                int h2, w2;
                if (odd) { w2 = l / g.H2; h2 = l - w2 * g.H2; }
                else { h2 = l / g.W2; w2 = l - h2 * g.W2; }
                const int hh = 2 * h2 + ph, ww = 2 * w2 + pw;
                const bool inimg = l < l1 && hh < g.H && ww < g.W;      // odd sizes: padded positions are zero rows
                const float *px = ubx + ((int64_t)hh * g.W + ww) * g.D + 8 * fg;
                const int lrow = h2 * g.W2 + w2;
                bf16x8 bh[KSM], bl[KSM];
#pragma unroll
                for (int ks = 0; ks < KSM; ++ks) {
                    float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    if (ks < nks && inimg) load8(px + 32 * ks, f);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const bf16 hv = (bf16)f[e];
                        bh[ks][e] = hv;
                        bl[ks][e] = (bf16)(f[e] - (float)hv);
                    }
                }
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) {
                    const int e = mb * 16 + fr;
                    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < KSM; ++ks) {
                        if (ks < nks) {
                            float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                            if (e < CD) load8(Wk + (int64_t)e * g.D + 32 * ks + 8 * fg, f);
                            bf16x8 ah, al;
#pragma unroll
                            for (int q = 0; q < 8; ++q) {
                                const bf16 hv = (bf16)f[q];
                                ah[q] = hv;
                                al[q] = (bf16)(f[q] - (float)hv);
                            }
                            acc = FD_MFMA16(al, bh[ks], acc, 0, 0, 0);
                            acc = FD_MFMA16(ah, bl[ks], acc, 0, 0, 0);
                            acc = FD_MFMA16(ah, bh[ks], acc, 0, 0, 0);
                        }
                    }
                    const int e0 = mb * 16 + 4 * fg;                    // CD % 4 == 0 (launcher): all four or none
                    if (l < l1 && e0 < CD) {
                        *(f32x4 *)&sx[(nb * 16 + fr) * CDP + e0] = acc;
                        *(f32x4 *)&xo[(int64_t)lrow * CD + e0] = acc;
                    }
                }
            }
        }
    }
    // ---- stage the chunk's rows (phase A with the fused x_proj writes them itself)
    if (FINAL || !g.xw)
    for (int idx = threadIdx.x; idx < (l1 - l0) * CD; idx += blockDim.x) {
        const int row = idx / CD, e = idx - row * CD;
        const int l = l0 + row;
        int h2, w2;
        if (odd) { w2 = l / g.H2; h2 = l - w2 * g.H2; }
        else { h2 = l / g.W2; w2 = l - h2 * g.W2; }
        float v = xb[(int64_t)(h2 * g.W2 + w2) * CD + e];
        // bf16 mode keeps dt in base-2 units (see `step`): the missing ln2 of dt*u is applied once per
        // staged C element instead of once per (step, channel)
        if (LOG2U && FINAL && e >= R + N) v *= 0.6931471805599453f;
        sx[row * CDP + e] = v;
    }

    // state / weights as float pairs: the recurrence runs on v_pk_mul_f32 / v_pk_fma_f32 (two states
    // per instruction at the scalar-op issue rate); only the two v_exp_f32 per pair stay scalar
    // CPL == 1: pair = (state 2n, 2n+1) of one channel, NP = N/2 pairs.  CPL == 2: pair = (channel d, d+1), NP = N.
    constexpr int NP = CPL == 2 ? N : N / 2, RP = CPL == 2 ? R : R / 2;
    f32x2 w[RP], a2[NP], h[NP];
    f32x2 bias2 = {0.f, 0.f}, Dd2 = {0.f, 0.f};
    float bias = 0.f, Dd = 0.f;
    const int64_t cbase = (((int64_t)bk * g.nch + chunk) * N) * g.D + d;   // [bk][chunk][n][d]
    if constexpr (CPL == 2) {
#pragma unroll
        for (int r = 0; r < R; ++r) w[r] = f32x2{dtw[(int64_t)kd * R + r], dtw[(int64_t)(kd + 1) * R + r]} * WS;
#pragma unroll
        for (int n = 0; n < N; ++n) a2[n] = f32x2{A[(int64_t)kd * N + n], A[(int64_t)(kd + 1) * N + n]} * AS;
        bias2 = f32x2{dtb[kd], dtb[kd + 1]} * WS;
        if (FINAL) Dd2 = f32x2{Ds[kd], Ds[kd + 1]};
#pragma unroll
        for (int n = 0; n < N; ++n) h[n] = FINAL ? *(const f32x2 *)&wsH[cbase + (int64_t)n * g.D] : f32x2{0.f, 0.f};
    } else {
#pragma unroll
        for (int r = 0; r < R / 2; ++r) w[r] = f32x2{dtw[(int64_t)kd * R + 2 * r], dtw[(int64_t)kd * R + 2 * r + 1]} * WS;
        // exp(dt*A) = exp2(dt * A*log2(e)): fold the constant into A once (v_exp_f32 is exp2)
#pragma unroll
        for (int n = 0; n < N / 2; ++n)
            a2[n] = f32x2{A[(int64_t)kd * N + 2 * n], A[(int64_t)kd * N + 2 * n + 1]} * AS;
        bias = dtb[kd] * WS;
        Dd = FINAL ? Ds[kd] : 0.f;
        if (FINAL) {
#pragma unroll
            for (int n = 0; n < N / 2; ++n)
                h[n] = f32x2{wsH[cbase + (int64_t)(2 * n) * g.D], wsH[cbase + (int64_t)(2 * n + 1) * g.D]};
        } else {
#pragma unroll
            for (int n = 0; n < N / 2; ++n) h[n] = f32x2{0.f, 0.f};
        }
    }
    float sdt = 0.f;
    f32x2 sdt2 = {0.f, 0.f};
    // wave-uniform row base + per-lane channel index: the row address stays on the scalar unit and the
    // loads/stores use the (sgpr base, vgpr offset) form -- no 64-bit vector address math per step
    // u / y rows through raw buffer descriptors: address = image base (SGPRs of the descriptor) + scalar
    // row offset (soffset) + the lane's constant channel offset -- no per-step VALU address arithmetic
    const T *ub = xc + (int64_t)b * g.H * g.W * g.D;
    T *yb = FINAL ? y + (int64_t)b * g.H * g.W * g.D : nullptr;
    const int rowb = g.D * (int)sizeof(T);
    const int img_bytes = g.H * g.W * rowb;
    const __amdgpu_buffer_rsrc_t rs_u = __builtin_amdgcn_make_buffer_rsrc((void *)ub, 0, img_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_y = __builtin_amdgcn_make_buffer_rsrc((void *)(FINAL ? yb : (T *)ub), 0, img_bytes, 0x00020000);
    const int voff = d * (int)sizeof(T);
    // u stays RAW (the 16 / 32 bits as loaded) until the step that uses it: converted at load time, the wait for a
    // whole group's loads sat in front of the previous group's steps -- the prefetch overlapped nothing
    auto ld_u = [&](int soff_) -> uint32_t {
        const int soff = __builtin_amdgcn_readfirstlane(soff_);     // uniform by construction; keeps the offset an SGPR
        if (ODD && soff < 0) return 0u;                // padded position (wave-uniform)
        if constexpr (CPL == 2) return __builtin_amdgcn_raw_buffer_load_b32(rs_u, voff, soff, 0);     // two bf16 channels
        else if constexpr (sizeof(T) == 2) return (uint32_t)__builtin_amdgcn_raw_buffer_load_b16(rs_u, voff, soff, 0);
        else return __builtin_amdgcn_raw_buffer_load_b32(rs_u, voff, soff, 0);
    };
    auto cvt_u = [&](uint32_t r) -> float {
        if constexpr (sizeof(T) == 2) return fd_h_lo(r);
        else return __builtin_bit_cast(float, r);
    };
    auto st_y = [&](int soff_, float v) {
        const int soff = __builtin_amdgcn_readfirstlane(soff_);     // (a VGPR offset turns the store into a waterfall loop)
        if (ODD && soff < 0) return;
        if constexpr (sizeof(T) == 2) {
            const bf16 hv = fd_cvt_h(v);
            __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, hv), rs_y, voff, soff, 0);
        } else {
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), rs_y, voff, soff, 0);
        }
    };
    auto st_y2 = [&](int soff_, f32x2 v) {
        const int soff = __builtin_amdgcn_readfirstlane(soff_);
        if (ODD && soff < 0) return;
        typedef __attribute__((ext_vector_type(2))) bf16 bfx2;
        const bfx2 hv = {fd_cvt_h(v.x), fd_cvt_h(v.y)};
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, hv), rs_y, voff, soff, 0);
    };
    // scan position -> (h2, w2) kept as scalar counters: no division in the loop
    // The integer division is computed on the vector unit; readfirstlane moves the (uniform) result to
    // SGPRs, otherwise everything derived from it (counters, wrap tests, row addresses) is treated as
    // divergent: exec-mask branches and 64-bit VALU address math in every step.
    // Branch-free walk: fast index i in [0, NI), slow index o; pix = base + i*s_i + o*s_o.
    const int NI = odd ? g.H2 : g.W2;
    const int s_i = odd ? 2 * g.W : 2, s_o = odd ? 2 : 2 * g.W;
    int ci = __builtin_amdgcn_readfirstlane(l0 % NI);
    int pixc = __builtin_amdgcn_readfirstlane(ph * g.W + pw + (l0 % NI) * s_i + (l0 / NI) * s_o);
    const int wrap_fix = s_o - NI * s_i;
    // ODD: the last fast / slow index of a sub-grid whose parity offset falls outside the image is padding
    const int NO = odd ? g.W2 : g.H2;
    const bool padF = ODD && (odd ? ((g.H & 1) && ph) : ((g.W & 1) && pw));
    const bool padS = ODD && (odd ? ((g.W & 1) && pw) : ((g.H & 1) && ph));
    int co = __builtin_amdgcn_readfirstlane(l0 / NI);
    __syncthreads();

    // CPL == 2: a step's row ([dt_r | B | C], the C part only in phase C) comes in REGISTERS, read from LDS one step
    // ahead by run() below (phase A waited s_waitcnt lgkmcnt(0) in every step: the broadcast read sat directly in
    // front of its use, an LDS round trip per ~100-cycle step that only the other waves could cover)
    constexpr int NXV = CPL == 2 ? ((FINAL ? CD : R + N) + 3) / 4 : 1;
    struct RowV { f32x4 v[NXV]; };
    auto ld_row = [&](int li) -> RowV {
        RowV q;
#pragma unroll
        for (int c = 0; c < NXV; ++c) q.v[c] = *(const f32x4 *)&sx[li * CDP + 4 * c];
        return q;
    };
    auto step = [&](const float *xr_lds, const RowV &rq, uint32_t uraw, int soff) {
        if constexpr (CPL == 2) {
            // row = [dt_r (R) | B (N) | C (N)] broadcast scalars; every pair below is (channel d, channel d + 1)
            const auto xr = [&](int i) -> float { return rq.v[i >> 2][i & 3]; };
            const f32x2 u2 = {fd_h_lo(uraw), fd_h_hi(uraw)};
            f32x2 dv2 = bias2;
#pragma unroll
            for (int r = 0; r < R; ++r) dv2 = w[r] * xr(r) + dv2;
            f32x2 dt2;
            dt2.x = __builtin_amdgcn_logf(1.0f + __builtin_amdgcn_exp2f(fminf(dv2.x, 126.f)));
            dt2.y = __builtin_amdgcn_logf(1.0f + __builtin_amdgcn_exp2f(fminf(dv2.y, 126.f)));
            const f32x2 dtu2 = dt2 * u2;
            if (!FINAL) sdt2 += dt2;
            f32x2 acc2 = Dd2 * u2;
#pragma unroll
            for (int n = 0; n < N; ++n) {
                const f32x2 t = a2[n] * dt2;
                const f32x2 da = {__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)};
                h[n] = da * h[n] + dtu2 * xr(R + n);
                if (FINAL) acc2 = h[n] * xr(R + N + n) + acc2;
            }
            if (FINAL) st_y2(soff, acc2);
        } else {
        const float u = cvt_u(uraw);
        const f32x2 *xr2 = (const f32x2 *)xr_lds;      // row = [dt_r (R) | B (N) | C (N)], all even
        f32x2 dv2 = {bias, 0.f};
#pragma unroll
        for (int r = 0; r < R / 2; ++r) dv2 = w[r] * xr2[r] + dv2;
        const float dv = dv2.x + dv2.y;
        float dt;
        if constexpr (LOG2U) dt = __builtin_amdgcn_logf(1.0f + __builtin_amdgcn_exp2f(fminf(dv, 126.f)));
        else dt = fd_softplus_fast(dv);
        const float dtu = dt * u;
        if (!FINAL) sdt += dt;
        f32x2 acc2 = {0.f, 0.f};
#pragma unroll
        for (int n = 0; n < N / 2; ++n) {
            const f32x2 t = a2[n] * dt;
            const f32x2 da = {__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)};
            h[n] = da * h[n] + xr2[R / 2 + n] * dtu;
            if (FINAL) acc2 = h[n] * xr2[R / 2 + N / 2 + n] + acc2;
        }
        if (FINAL) st_y(soff, acc2.x + acc2.y + Dd * u);
        }
    };
    auto advance = [&](int &soff) {            // -> byte offset of the pixel's row inside the image (-1: padding)
        soff = pixc * rowb;
        if (ODD && ((padF && ci == NI - 1) || (padS && co == NO - 1))) soff = -1;
        ++ci;
        const bool wrap = ci == NI;
        ci = wrap ? 0 : ci;
        if (ODD) co += wrap ? 1 : 0;
        pixc += s_i + (wrap ? wrap_fix : 0);
    };
    // ---- phase A, two channels per lane (one wave = all 128 channels of the chunk), fused x_proj: ONE read of u (round 5).
    // Block by block (16 positions): the block's pixels arrive as MFMA B fragments (lane (fr, fg): pixel fr, channels
    // 32 ks + 8 fg ..), the x_proj rows go from the accumulators into sx (and out to x_dbl for phase C), the SAME
    // fragments are parked in a 4 KB LDS block [16 positions][128 channels] and the 16 recurrence steps read their u pair
    // from there (ds_read_b32) -- the recurrence issues no global load at all, the next block's fragments are in flight in
    // registers meanwhile.  Until round 4 the whole chunk's x_proj ran first and the recurrence re-read every u from
    // global memory up to 128 steps (~12 us) later: an XCD's L2 turns over in ~3 us (tools/probes/fetch_calib.hip), so that
    // second read went back to HBM (FETCH_SIZE of this phase = 2 x u).  Same MFMAs on the same operands in the same order,
    // same u bits: results are bitwise those of the two-read form.
    if constexpr (!FINAL && CPL == 2) {
        if (g.xw) {
            unsigned char *su = (unsigned char *)(sx + g.CL * CDP);            // [16][256 B], 16-byte chunks XOR (row & 15)
            const bf16 *Wk = (const bf16 *)g.xw + (int64_t)k * CD * g.D;
            const bf16 *ubx = (const bf16 *)xc + (int64_t)b * g.H * g.W * g.D;
            float *xo = g.xdbl_out + ((int64_t)k * g.B + b) * g.L * g.CD;
            constexpr int MB = (CD + 15) / 16, KSM = 4;                       // d_inner == 128 (launcher)
            const int fr = lane & 15, fg = lane >> 4;
            const int nblk = (l1 - l0 + 15) >> 4;
            struct BlkPos { int l, lrow; };
            auto bfetch = [&](int nb, BlkPos &q, bf16x8 (&bq)[KSM]) {
                const int l = l0 + nb * 16 + fr;
                int h2, w2;
                if (odd) { w2 = l / g.H2; h2 = l - w2 * g.H2; }
                else { h2 = l / g.W2; w2 = l - h2 * g.W2; }
                const int hh = 2 * h2 + ph, ww = 2 * w2 + pw;
                const bool inimg = l < l1 && hh < g.H && ww < g.W;          // odd sizes: padded positions are zero rows, u = 0
                const bf16 *px = ubx + ((int64_t)hh * g.W + ww) * g.D + 8 * fg;
                q.l = l;
                q.lrow = h2 * g.W2 + w2;
#pragma unroll
                for (int ks = 0; ks < KSM; ++ks) {
                    bq[ks] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
                    if (inimg) bq[ks] = *(const bf16x8 *)(px + 32 * ks);
                }
            };
            // the weight fragments of the chunk's direction: MB x 4 x 16 bytes per lane, loaded once (they were re-read from
            // L2 for every block)
            bf16x8 afr[MB][KSM];
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                const int e = mb * 16 + fr;
#pragma unroll
                for (int ks = 0; ks < KSM; ++ks) {
                    afr[mb][ks] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
                    if (e < CD) afr[mb][ks] = *(const bf16x8 *)(Wk + (int64_t)e * g.D + 32 * ks + 8 * fg);
                }
            }
            // this lane's u pair of block position s: channels 2 lane, 2 lane + 1 = bytes 4 lane .. of row s
            const int su_rd = ((lane >> 2) << 4) | ((lane & 3) << 2);
            auto ld_su = [&](int s_) -> uint32_t { return *(const uint32_t *)(su + s_ * 256 + (su_rd ^ ((s_ & 15) << 4))); };
            BlkPos cur, nxt;
            bf16x8 bcur[KSM], bnxt[KSM];
            bfetch(0, cur, bcur);
            for (int nb = 0; nb < nblk; ++nb) {
                const bool more = nb + 1 < nblk;
                if (more) bfetch(nb + 1, nxt, bnxt);
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) {
                    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < KSM; ++ks) acc = FD_MFMA16(afr[mb][ks], bcur[ks], acc, 0, 0, 0);
                    const int e0 = mb * 16 + 4 * fg;                        // CD % 4 == 0 (launcher): all four or none
                    if (cur.l < l1 && e0 < CD) {
                        *(f32x4 *)&sx[(nb * 16 + fr) * CDP + e0] = acc;
                        *(f32x4 *)&xo[(int64_t)cur.lrow * CD + e0] = acc;
                    }
                }
#pragma unroll
                for (int ks = 0; ks < KSM; ++ks) *(bf16x8 *)(su + fr * 256 + (((ks * 4 + fg) ^ fr) << 4)) = bcur[ks];
                const int ns = min(16, l1 - l0 - nb * 16);                  // wave-uniform
                if (ns == 16) {
                    RowV r0 = ld_row(nb * 16);
                    uint32_t u0 = ld_su(0);
#pragma unroll
                    for (int st = 0; st < 16; ++st) {
                        RowV r1 = r0;
                        uint32_t u1 = u0;
                        if (st + 1 < 16) { r1 = ld_row(nb * 16 + st + 1); u1 = ld_su(st + 1); }
                        __builtin_amdgcn_sched_barrier(0);                  // the reads stay a step ahead of their use
                        step(nullptr, r0, u0, 0);
                        r0 = r1;
                        u0 = u1;
                    }
                } else {
                    for (int st = 0; st < ns; ++st) step(nullptr, ld_row(nb * 16 + st), ld_su(st), 0);
                }
                if (more) {
                    cur = nxt;
#pragma unroll
                    for (int ks = 0; ks < KSM; ++ks) bcur[ks] = bnxt[ks];
                }
            }
#pragma unroll
            for (int n = 0; n < N; ++n) *(f32x2 *)&wsH[cbase + (int64_t)n * g.D] = h[n];
            *(f32x2 *)&wsP[((int64_t)bk * g.nch + chunk) * g.D + d] = sdt2;
            return;
        }
    }
    constexpr int U = (N >= 16) ? 8 : 16;  // steps per group
    // Two groups of u values in registers: group g+1 is loaded while group g runs the recurrence, so a
    // wave always has U loads in flight behind ~U steps of arithmetic (HBM latency under load is longer
    // than one group's compute; 4 waves per SIMD alone do not cover it).
    int l = l0;
    const int ngroups = (l1 - l0) / U;
    int pixA[U], pixB[U];
    uint32_t uA[U], uB[U];
    auto fetch = [&](int (&pix)[U], uint32_t (&u)[U]) {
#pragma unroll
        for (int s = 0; s < U; ++s) advance(pix[s]);
#pragma unroll
        for (int s = 0; s < U; ++s) u[s] = ld_u(pix[s]);
    };
    auto run = [&](const int (&pix)[U], const uint32_t (&u)[U]) {
        if constexpr (CPL == 2) {
            RowV r0 = ld_row(l - l0);
#pragma unroll
            for (int s = 0; s < U; ++s) {
                RowV r1 = r0;
                if (s + 1 < U) r1 = ld_row(l - l0 + s + 1);
                __builtin_amdgcn_sched_barrier(0);          // the read stays a step ahead of its use
                step(nullptr, r0, u[s], pix[s]);
                r0 = r1;
            }
        } else {
            const RowV none = {};
#pragma unroll
            for (int s = 0; s < U; ++s) step(sx + (l - l0 + s) * CDP, none, u[s], pix[s]);
        }
        l += U;
    };
    if (ngroups > 0) fetch(pixA, uA);
    for (int gi = 0; gi < ngroups; gi += 2) {
        if (gi + 1 < ngroups) fetch(pixB, uB);
        run(pixA, uA);
        if (gi + 1 < ngroups) {
            if (gi + 2 < ngroups) fetch(pixA, uA);
            run(pixB, uB);
        }
    }
    for (; l < l1; ++l) {
        int soff;
        advance(soff);
        step(sx + (l - l0) * CDP, ld_row(l - l0), ld_u(soff), soff);
    }
    if (!FINAL) {
        // chunk decay P[n] = exp2(a2[n] * sum dt): only the sum is stored ([bk][chunk][d], N x smaller than
        // P itself); the carry kernel rebuilds P from it -- at the 64x64 levels (N = 32, 32-step chunks)
        // the P/H workspace traffic was 4x the u/y traffic of the scan
        if constexpr (CPL == 2) {
#pragma unroll
            for (int n = 0; n < N; ++n) *(f32x2 *)&wsH[cbase + (int64_t)n * g.D] = h[n];
            *(f32x2 *)&wsP[((int64_t)bk * g.nch + chunk) * g.D + d] = sdt2;
        } else {
#pragma unroll
            for (int n = 0; n < N / 2; ++n) {
                wsH[cbase + (int64_t)(2 * n) * g.D] = h[n].x;
                wsH[cbase + (int64_t)(2 * n + 1) * g.D] = h[n].y;
            }
            wsP[((int64_t)bk * g.nch + chunk) * g.D + d] = sdt;
        }
    }
}

// Phase B: block = 64 channels x S segments.  Each segment composes its chunks, segments are
// chained through LDS, then each segment rewrites H_c with the carry-in of chunk c.
constexpr int SEG = 16;
// PER = chunks per segment (compile-time bound): a thread keeps its segment's (decay, H) pairs in registers
// between composing the segment and rewriting the carry-ins, so the chunk-state workspace is read ONCE and
// written once (it was read twice: this kernel is bandwidth-bound on that fp32 workspace -- N x D floats per
// chunk and direction, 540 us per batch-8 forward).
template <int PER>
__global__ __launch_bounds__(64 * SEG) void scan_carry_kernel(float *__restrict__ wsH, const float *__restrict__ wsS,
                                                             const float *__restrict__ A, float a_scale, int nch,
                                                             int N, int D) {
    __shared__ float sP[SEG][64], sH[SEG][64];
    const int lane = threadIdx.x & 63;
    const int seg = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int dblocks = D / 64;
    const int db = blockIdx.x % dblocks, n = (blockIdx.x / dblocks) % N, bk = blockIdx.x / (dblocks * N);
    const int d = db * 64 + lane;
    const int per = (nch + SEG - 1) / SEG;              // <= PER (launcher)
    const int c0 = seg * per, c1 = min(c0 + per, nch);
    const int64_t base = ((int64_t)bk * nch * N + n) * D + d;   // + c*N*D
    const int64_t cs = (int64_t)N * D;
    const float *sd = wsS + (int64_t)bk * nch * D + d;          // + c*D: sum of dt of chunk c
    const float a2 = A[((int64_t)(bk & 3) * D + d) * N + n] * a_scale;
    if constexpr (PER == 0) {       // segments longer than 8 chunks (small state, N <= 8, or huge images): two passes over
                                    // the workspace -- 2 x 32 register-held values do not fit a 1024-thread workgroup
        float P = 1.f, Hh = 0.f;
        for (int c = c0; c < c1; ++c) {
            const float p = __builtin_amdgcn_exp2f(a2 * sd[(int64_t)c * D]), hh = wsH[base + c * cs];
            Hh = p * Hh + hh;
            P = p * P;
        }
        sP[seg][lane] = P;
        sH[seg][lane] = Hh;
        __syncthreads();
        float carry = 0.f;
        for (int s = 0; s < seg; ++s) carry = sP[s][lane] * carry + sH[s][lane];
        for (int c = c0; c < c1; ++c) {
            const float p = __builtin_amdgcn_exp2f(a2 * sd[(int64_t)c * D]), hh = wsH[base + c * cs];
            wsH[base + c * cs] = carry;
            carry = p * carry + hh;
        }
        return;
    }
    constexpr int PR = PER > 0 ? PER : 1;
    float pv[PR], hv[PR];
    // running pointers (one live address each): 2 x PER precomputed 64-bit addresses would not fit the
    // 128 VGPRs of a 1024-thread workgroup
    const float *ps = sd + (int64_t)c0 * D;
    float *ph = wsH + base + c0 * cs;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        pv[u] = 0.f;
        hv[u] = 0.f;
        if (c0 + u < c1) {                              // wave-uniform
            pv[u] = *ps;
            hv[u] = *ph;
        }
        ps += D;
        ph += cs;
    }
    float P = 1.f, Hh = 0.f;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        if (c0 + u < c1) {
            pv[u] = __builtin_amdgcn_exp2f(a2 * pv[u]);
            Hh = pv[u] * Hh + hv[u];
            P = pv[u] * P;
        }
    }
    sP[seg][lane] = P;
    sH[seg][lane] = Hh;
    __syncthreads();
    float carry = 0.f;
    for (int s = 0; s < seg; ++s) carry = sP[s][lane] * carry + sH[s][lane];
    ph = wsH + base + c0 * cs;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        if (c0 + u < c1) {
            *ph = carry;
            carry = pv[u] * carry + hv[u];
        }
        ph += cs;
    }
}

// ---- Single-pass scan for short sequences with a wide state (L <= 1024 and N >= 16: the 64x64 level of a 512x512
// slice, N = 32; levels 2-3 of a 256x256 slice).  The chunked form above runs the recurrence TWICE (local scan, then
// the re-run from the carry-in: every exp2, softplus and dt_proj a second time) and, with 32-step chunks and N = 32,
// moves 4x the u / y bytes through its fp32 chunk-state workspace (N floats per channel and chunk, written, carried,
// read back).  Where the state is wide the parallelism is in the STATE: SEQ_LPC = 4 neighbouring lanes share one
// channel, each owns N/4 states and R/4 of the dt_proj contraction, and the sequence is walked once from h = 0 -- no
// chunks, no workspace, no carry kernel.  Per step: dt_proj partial (R/4 FMAs) + quad all-reduce (2 DPP adds),
// softplus (replicated in the 4 lanes), N/4 state updates as float pairs, y partial + quad all-reduce, lane 0 of the
// quad stores.  The x_dbl rows of SEQ_SP positions are staged in LDS (double buffer, the next block's global loads in
// flight during the current block's steps); each lane reads its own slices of a row: 4 distinct addresses per
// ds_read.  Which path runs is a function of (H, W, N, R) only -- never of the batch -- so a slice's result does not
// depend on what else is in the batch (scan_seq_ok).
// (Round 6, measured and not kept: 8 lanes per channel at N = 32 -- half the states per lane, twice the waves, each lane of the octet
// computing the dt of one of 8 steps, the cross-quad broadcast through the half-row mirror DPP.  VERDICT r5 expected the one-wave-
// per-SIMD d_inner 512 launch (VALU 46 % busy) to gain; batch-8 launches, alternated in one call: d_inner 512 201 -> 204-207 us,
// d_inner 1024 289 -> 376-380 us.  The per-step work that does NOT shrink with the state slice -- u conversion, the y all-reduce
// (3 instead of 2 DPP adds), broadcast moves, the store, row reads -- is paid by twice as many lanes: issue-bound, not latency-bound.)
constexpr int SEQ_LPC = 4, SEQ_SP = 32, SEQ_MAXL = 1024;

__device__ __forceinline__ float quad_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));   // lane ^ 1
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));   // lane ^ 2
    return v;
}

template <typename T, int N, int R, bool ODD>
__global__ __launch_bounds__(256) void scan_seq_kernel(const T *__restrict__ xc, const float *__restrict__ xdbl,
                                                      const float *__restrict__ dtw, const float *__restrict__ dtb,
                                                      const float *__restrict__ A, const float *__restrict__ Ds,
                                                      T *__restrict__ y, const ScanGeom g) {
    constexpr int LPC = SEQ_LPC, NS = N / LPC, RS = R / LPC, SP = SEQ_SP;
    constexpr int CD = R + 2 * N, CD4 = CD / 4;
    static_assert(NS % 2 == 0 && RS % 2 == 0 && CD % 4 == 0 && (R + N) % 4 == 0, "scan_seq_kernel: slice shapes");
    constexpr bool LOG2U = sizeof(T) == 2;                           // see scan_chunk_kernel: dt in base-2 units
    constexpr float WS = LOG2U ? 1.4426950408889634f : 1.f;
    constexpr float AS = LOG2U ? 1.f : 1.4426950408889634f;
    // LDS row stride: the four lanes of a quad read the dt_r parts of four DIFFERENT rows (dt_of_row); with a stride of
    // CD = 96 floats all four fall on the same banks (PMC: 24 % of the LDS cycles were conflicts)
    constexpr int CDS = CD + 4;
    __shared__ __attribute__((aligned(16))) float sx[2][SP * CDS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int sub = lane & 3;
    const int bk = blockIdx.y, b = bk >> 2, k = bk & 3;
    const int d = blockIdx.x * 64 + wave * 16 + (lane >> 2);
    const int kd = k * g.D + d;
    const int odd = k & 1, ph = k & 1, pw = k >> 1;
    const float *xb = xdbl + ((int64_t)k * g.B + b) * g.L * CD;       // [4][B][L][CD], row = h2 * W2 + w2

    // dt_proj: every lane holds the channel's FULL rank-R weight row -- the four lanes of a quad compute the dt of four
    // DIFFERENT steps each (dt_of_row below) instead of a quarter of every step's contraction plus a quad all-reduce and
    // a 4x replicated softplus: 28 instead of 56 lane-slots per (channel, position)
    f32x2 w[R / 2], a2[NS / 2], h[NS / 2];
#pragma unroll
    for (int r = 0; r < R / 2; ++r)
        w[r] = f32x2{dtw[(int64_t)kd * R + 2 * r], dtw[(int64_t)kd * R + 2 * r + 1]} * WS;
#pragma unroll
    for (int n = 0; n < NS / 2; ++n) {
        a2[n] = f32x2{A[(int64_t)kd * N + sub * NS + 2 * n], A[(int64_t)kd * N + sub * NS + 2 * n + 1]} * AS;
        h[n] = f32x2{0.f, 0.f};
    }
    const float bias = dtb[kd] * WS;
    const float Dd = Ds[kd];

    const T *ub = xc + (int64_t)b * g.H * g.W * g.D;
    T *yb = y + (int64_t)b * g.H * g.W * g.D;
    const int rowb = g.D * (int)sizeof(T);
    const int img_bytes = g.H * g.W * rowb;
    const __amdgpu_buffer_rsrc_t rs_u = __builtin_amdgcn_make_buffer_rsrc((void *)ub, 0, img_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_y = __builtin_amdgcn_make_buffer_rsrc((void *)yb, 0, img_bytes, 0x00020000);
    const int voff = d * (int)sizeof(T);
    // u is kept RAW (16 / 32 bits as loaded) until the step that uses it: converting at load time puts the wait for
    // the whole group's loads in front of the previous group's steps
    auto ld_u = [&](int soff_) -> uint32_t {
        const int soff = __builtin_amdgcn_readfirstlane(soff_);
        if (ODD && soff < 0) return 0u;
        if constexpr (sizeof(T) == 2) return (uint32_t)__builtin_amdgcn_raw_buffer_load_b16(rs_u, voff, soff, 0);
        else return __builtin_amdgcn_raw_buffer_load_b32(rs_u, voff, soff, 0);
    };
    auto cvt_u = [&](uint32_t r) -> float {
        if constexpr (sizeof(T) == 2) return fd_h_lo(r);
        else return __builtin_bit_cast(float, r);
    };
    // all four lanes of a quad hold the same y (quad_sum is an all-reduce) and store it to the same address: no
    // exec-mask branch inside the unrolled group, one basic block for the scheduler
    auto st_y = [&](int soff_, float v) {
        // the offsets are wave-uniform by construction; when the register allocator parks a group's offsets in VGPRs
        // across the loop back-edge the store would otherwise become a waterfall loop
        const int soff = __builtin_amdgcn_readfirstlane(soff_);
        if (ODD && soff < 0) return;
        if constexpr (sizeof(T) == 2) {
            const bf16 hv = fd_cvt_h(v);
            __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, hv), rs_y, voff, soff, 0);
        } else {
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), rs_y, voff, soff, 0);
        }
    };
    // scan position -> pixel: the branch-free scalar walk of scan_chunk_kernel, from l = 0
    const int NI = odd ? g.H2 : g.W2;
    const int s_i = odd ? 2 * g.W : 2, s_o = odd ? 2 : 2 * g.W;
    int ci = 0, co = 0;
    int pixc = __builtin_amdgcn_readfirstlane(ph * g.W + pw);
    const int wrap_fix = s_o - NI * s_i;
    const int NO = odd ? g.W2 : g.H2;
    const bool padF = ODD && (odd ? ((g.H & 1) && ph) : ((g.W & 1) && pw));
    const bool padS = ODD && (odd ? ((g.W & 1) && pw) : ((g.H & 1) && ph));
    auto advance = [&](int &soff) {
        soff = pixc * rowb;
        if (ODD && ((padF && ci == NI - 1) || (padS && co == NO - 1))) soff = -1;
        ++ci;
        const bool wrap = ci == NI;
        ci = wrap ? 0 : ci;
        if (ODD) co += wrap ? 1 : 0;
        pixc += s_i + (wrap ? wrap_fix : 0);
    };

    // staged x_dbl rows: block st = positions [st * SP, ...), row r of the block = [dt_r | B | C] of position st*SP + r
    constexpr int NLD = (SP * CD4 + 255) / 256;
    f32x4 stg[NLD];
    auto load_rows = [&](int st) {
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int idx = tid + j * 256;
            const int r = idx / CD4, e4 = idx - r * CD4;
            const int l = st * SP + r;
            stg[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (idx < SP * CD4 && l < g.L) {
                int h2, w2;
                if (odd) { w2 = l / g.H2; h2 = l - w2 * g.H2; }
                else { h2 = l / g.W2; w2 = l - h2 * g.W2; }
                f32x4 v = *(const f32x4 *)(xb + (int64_t)(h2 * g.W2 + w2) * CD + 4 * e4);
                if (LOG2U && 4 * e4 >= R + N) v = v * 0.6931471805599453f;    // the ln2 of dt*u, once per C element
                stg[j] = v;
            }
        }
    };
    auto store_rows = [&](int buf) {
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int idx = tid + j * 256;
            if (idx < SP * CD4) *(f32x4 *)&sx[buf][(idx / CD4) * CDS + 4 * (idx % CD4)] = stg[j];
        }
    };
    auto lds_barrier = [&]() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };

    // a step's slices of its x_dbl row, in registers: loaded one step ahead of their use (the LDS round trip of a
    // read issued right before its consumer was most of a step's time at one or two waves per SIMD)
    struct RowRegs { f32x2 br[NS / 2], cr[NS / 2]; };
    auto load_row = [&](const float *xr, RowRegs &q) {
        const f32x2 *br2 = (const f32x2 *)(xr + R + sub * NS);
        const f32x2 *cr2 = (const f32x2 *)(xr + R + N + sub * NS);
#pragma unroll
        for (int n = 0; n < NS / 2; ++n) { q.br[n] = br2[n]; q.cr[n] = cr2[n]; }
    };
    // dt of the position whose row is `xr`: the whole contraction + softplus in this lane
    auto dt_of_row = [&](const float *xr) -> float {
        const f32x2 *wr2 = (const f32x2 *)xr;
        f32x2 dv2 = {0.f, 0.f}, dv3 = {0.f, 0.f};
#pragma unroll
        for (int r = 0; r < R / 2; ++r) {
            if (r & 1) dv3 = w[r] * wr2[r] + dv3;
            else dv2 = w[r] * wr2[r] + dv2;
        }
        const float dv = ((dv2.x + dv3.x) + (dv2.y + dv3.y)) + bias;
        if constexpr (LOG2U) return __builtin_amdgcn_logf(1.0f + __builtin_amdgcn_exp2f(fminf(dv, 126.f)));
        else return fd_softplus_fast(dv);
    };
    // A step in two halves.  pre(): everything that does not depend on the state -- the N/4 decay factors exp2(A dt) and
    // inputs B dt u (dt: this step's lane of the quad, broadcast).  post(): the recurrence itself, the C contraction,
    // the quad all-reduce of y and the store.  run() issues pre(s + 1) next to post(s): two independent dependency
    // chains for the scheduler to interleave (a lone wave spent ~500 cycles per step walking one chain of ~30
    // dependent instructions; the state update is only the last third of it).
    struct PreOut { f32x2 da[NS / 2], bdu[NS / 2]; float du; };
    auto pre = [&](const RowRegs &q, uint32_t uraw, float dt, PreOut &o) {
        const float u = cvt_u(uraw);
        const float dtu = dt * u;
        o.du = Dd * u;
#pragma unroll
        for (int n = 0; n < NS / 2; ++n) {
            const f32x2 t = a2[n] * dt;
            o.da[n] = f32x2{__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)};
            o.bdu[n] = q.br[n] * dtu;
        }
    };
    auto post = [&](const RowRegs &q, const PreOut &o, int soff) {
        f32x2 acc2 = {0.f, 0.f}, acc3 = {0.f, 0.f};
#pragma unroll
        for (int n = 0; n < NS / 2; ++n) {
            h[n] = o.da[n] * h[n] + o.bdu[n];
            if (n & 1) acc3 = h[n] * q.cr[n] + acc3;
            else acc2 = h[n] * q.cr[n] + acc2;
        }
        st_y(soff, quad_sum((acc2.x + acc3.x) + (acc2.y + acc3.y)) + o.du);
    };

    constexpr int U = 8;                                 // steps per prefetch group; SP / U groups per staged block
    const int G = g.L / U;
    int pixA[U], pixB[U];
    uint32_t uA[U], uB[U];
    auto fetch = [&](int (&pix)[U], uint32_t (&u)[U]) {
#pragma unroll
        for (int s = 0; s < U; ++s) advance(pix[s]);
#pragma unroll
        for (int s = 0; s < U; ++s) u[s] = ld_u(pix[s]);
    };
    // lane `sub` of a quad -> the value lane i of the quad holds (i: compile-time)
    auto quad_bcast = [&](float v, int i) -> float {
        const int x = __builtin_bit_cast(int, v);
        int r;
        if (i == 0) r = __builtin_amdgcn_update_dpp(0, x, 0x00, 0xF, 0xF, true);
        else if (i == 1) r = __builtin_amdgcn_update_dpp(0, x, 0x55, 0xF, 0xF, true);
        else if (i == 2) r = __builtin_amdgcn_update_dpp(0, x, 0xAA, 0xF, 0xF, true);
        else r = __builtin_amdgcn_update_dpp(0, x, 0xFF, 0xF, 0xF, true);
        return __builtin_bit_cast(float, r);
    };
    auto run = [&](int gi, const int (&pix)[U], const uint32_t (&u)[U]) {
        const float *rows = &sx[(gi >> 2) & 1][((gi & 3) * U) * CDS];
        RowRegs q[3];
        PreOut o[2];
        float dtq[U / 4];                                // dt of step 4 b + sub of block b, in lane `sub`
        load_row(rows, q[0]);
        load_row(rows + CDS, q[1]);
        dtq[0] = dt_of_row(rows + sub * CDS);
        pre(q[0], u[0], quad_bcast(dtq[0], 0), o[0]);
#pragma unroll
        for (int s = 0; s < U; ++s) {
            if (s + 2 < U) load_row(rows + (s + 2) * CDS, q[(s + 2) % 3]);
            __builtin_amdgcn_sched_barrier(0);           // the reads stay two steps ahead of their use
            if ((s & 3) == 0 && s + 4 < U) dtq[s / 4 + 1] = dt_of_row(rows + (s + 4 + sub) * CDS);    // next block's dt
            if (s + 1 < U) pre(q[(s + 1) % 3], u[s + 1], quad_bcast(dtq[(s + 1) / 4], (s + 1) & 3), o[(s + 1) & 1]);
            post(q[s % 3], o[s & 1], pix[s]);
        }
    };
    load_rows(0);
    store_rows(0);
    if (SP < g.L) load_rows(1);
    if (G > 0) fetch(pixA, uA);
    lds_barrier();
    for (int gi = 0; gi < G; gi += 2) {
        if (gi + 1 < G) fetch(pixB, uB);
        run(gi, pixA, uA);
        if (gi + 1 < G) {
            if (gi + 2 < G) fetch(pixA, uA);
            run(gi + 1, pixB, uB);
            if ((gi & 3) == 2) {                          // staged block gi / 4 is done
                const int st = gi >> 2;
                if ((st + 1) * SP < g.L) store_rows((st + 1) & 1);
                lds_barrier();
                if ((st + 2) * SP < g.L) load_rows(st + 2);
            }
        }
    }
    for (int l = G * U; l < g.L; ++l) {
        int soff;
        advance(soff);
        RowRegs q;
        PreOut o;
        const float *xr = &sx[(l / SP) & 1][(l % SP) * CDS];
        load_row(xr, q);
        pre(q, ld_u(soff), dt_of_row(xr), o);
        post(q, o, soff);
    }
}

// the single-pass form applies to (image size, state size, rank) only: batch-invariant by construction
bool scan_seq_ok(int H, int W, int D, int N, int R) {
    const bool off = fd_dev(FD_DEV_SCAN_NO_SEQ);     // development switch: time the chunked form
    if (off) return false;
    const int L = ((H + 1) / 2) * ((W + 1) / 2);
    return L <= SEQ_MAXL && N >= 16 && N % (2 * SEQ_LPC) == 0 && R % (2 * SEQ_LPC) == 0 && D % 64 == 0;
}

template <typename T, int N, int R, bool ODD>
void launch_scan_seq(const T *xc, const float *xdbl, const float *dtw, const float *dtb, const float *A,
                     const float *Ds, T *y, const ScanGeom &g, hipStream_t s) {
    if constexpr (N >= 16 && N % (2 * SEQ_LPC) == 0 && R % (2 * SEQ_LPC) == 0) {
        dim3 grid(g.D / 64, g.B * 4), block(256);
        hipLaunchKernelGGL((scan_seq_kernel<T, N, R, ODD>), grid, block, 0, s, xc, xdbl, dtw, dtb, A, Ds, y, g);
    }
}

// the carry-ins of a single chunk: n zeros
__global__ __launch_bounds__(256) void scan_zero_kernel(float *__restrict__ p, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0.f;
}

static bool scan_cpl2_on() {
    const bool off = fd_dev(FD_DEV_SCAN_NO_CPL2);    // development switch
    return !off;
}

// Everything the launcher decides from the shape, in one place: launch_scan launches what this says and
// fd_selective_scan_geom reports it, so the tests' coverage table (tests/scan_cases.py) cannot drift from the launcher.
struct ScanPlan {
    bool seq;       // the single-pass form; nothing below applies to it
    bool two;       // two channels per lane
    int cw, nw;     // channels per wave, waves per workgroup
    int wgs;        // workgroups per chunk
    int carry;      // scan_carry_kernel's PER (2, 8, 0), or -1: a single chunk, the carry-ins are a memset
    size_t lds;     // dynamic LDS bytes of scan_chunk_kernel
};

// half: 16-bit storage; g.xw: the x_proj rows are computed inside phase A
ScanPlan scan_plan(const ScanGeom &g, bool half) {
    ScanPlan p = {};
    p.seq = !g.xw && !g.low_latency && scan_seq_ok(g.H, g.W, g.D, g.N, g.R);
    if (p.seq) return p;
    // two channels per lane where the kernel is VALU-bound and the state is small (bf16, N <= 8); a function of the
    // shape only
    const int cpl = (half && g.N <= 4) ? 2 : 1;        // N = 8: measured slower (305 vs 293 us at 256x256, batch 8)
    // (with the x_proj einsum inside phase A the two-channel form holds d_inner / 32 <= 4 pixel fragments per block)
    // (not for ONE slice: a lone image has 2048 two-channel waves at level 0 for 1024 SIMDs; one channel per lane doubles
    //  them: 155.7 -> 154.3 ms per 50-step slice at batch 1)
    p.two = cpl == 2 && g.D % 128 == 0 && (!g.xw || g.D == 128) && scan_cpl2_on() && !g.low_latency;
    p.cw = p.two ? 128 : 64;                           // channels per wave
    p.nw = g.D >= 4 * p.cw ? 4 : g.D / p.cw;           // waves per workgroup
    p.wgs = g.D / (p.cw * p.nw);
    const size_t pad = fd_occ_pad(FD_DEV_PAD_SCAN);
    // (+ 4 KB behind the rows: the u block of the two-channel phase A with the fused x_proj)
    p.lds = (size_t)g.CL * ((g.CD + 3) & ~3) * sizeof(float) + (p.two && g.xw ? 4096 : 0) + pad;
    const int per = (g.nch + SEG - 1) / SEG;           // chunks per segment of scan_carry_kernel
    p.carry = g.nch <= 1 ? -1 : per <= 2 ? 2 : per <= 8 ? 8 : 0;
    return p;
}

template <typename T, int N, int R, bool ODD>
void launch_scan(const T *xc, const float *xdbl, const float *dtw, const float *dtb, const float *A,
                 const float *Ds, T *y, float *ws, const ScanGeom &g, hipStream_t s) {
    const ScanPlan p = scan_plan(g, sizeof(T) == 2);
    if (p.seq) {
        launch_scan_seq<T, N, R, ODD>(xc, xdbl, dtw, dtb, A, Ds, y, g, s);
        return;
    }
    const int64_t half = (int64_t)g.B * 4 * g.nch * g.N * g.D;
    float *wsH = ws, *wsP = ws + half;
    constexpr int CPL = (sizeof(T) == 2 && N <= 4) ? 2 : 1;     // the only instantiation scan_plan's `two` can ask for
    const bool two = CPL == 2 && p.two;
    dim3 grid(g.nch * p.wgs, g.B * 4), block(64 * p.nw);
    const size_t lds = p.lds;
    if (two) hipLaunchKernelGGL((scan_chunk_kernel<T, N, R, false, ODD, CPL>), grid, block, lds, s, xc, xdbl, dtw, dtb, A, Ds, y, wsH, wsP, g);
    else hipLaunchKernelGGL((scan_chunk_kernel<T, N, R, false, ODD>), grid, block, lds, s, xc, xdbl, dtw, dtb, A, Ds, y, wsH, wsP, g);
    if (p.carry >= 0)
    {
        const dim3 cgrid(g.B * 4 * g.N * (g.D / 64)), cblock(64 * SEG);
        const float asc = sizeof(T) == 2 ? 1.f : 1.4426950408889634f;
        if (p.carry == 2) hipLaunchKernelGGL(scan_carry_kernel<2>, cgrid, cblock, 0, s, wsH, wsP, A, asc, g.nch, g.N, g.D);
        else if (p.carry == 8) hipLaunchKernelGGL(scan_carry_kernel<8>, cgrid, cblock, 0, s, wsH, wsP, A, asc, g.nch, g.N, g.D);
        else hipLaunchKernelGGL(scan_carry_kernel<0>, cgrid, cblock, 0, s, wsH, wsP, A, asc, g.nch, g.N, g.D);
    }
    else   // a kernel, not hipMemsetAsync: inside a captured loop graph the memset node left stale carry-ins in place (a level of
           // 16 x 16 pixels, the only shape with one chunk: a sample() there differed from capture to capture and from the eager loop)
        hipLaunchKernelGGL(scan_zero_kernel, dim3((unsigned)((half + 255) / 256)), dim3(256), 0, s, wsH, half);
    if (two) hipLaunchKernelGGL((scan_chunk_kernel<T, N, R, true, ODD, CPL>), grid, block, lds, s, xc, xdbl, dtw, dtb, A, Ds, y, wsH, wsP, g);
    else hipLaunchKernelGGL((scan_chunk_kernel<T, N, R, true, ODD>), grid, block, lds, s, xc, xdbl, dtw, dtb, A, Ds, y, wsH, wsP, g);
}

template <typename T, int N>
int dispatch_r(const T *xc, const float *xdbl, const float *dtw, const float *dtb, const float *A,
               const float *Ds, T *y, float *ws, const ScanGeom &g, hipStream_t s) {
    const bool oddsz = (g.H | g.W) & 1;
#define FD_SCAN_R(RR)                                                                            \
    case RR:                                                                                     \
        if (oddsz) launch_scan<T, N, RR, true>(xc, xdbl, dtw, dtb, A, Ds, y, ws, g, s);          \
        else launch_scan<T, N, RR, false>(xc, xdbl, dtw, dtb, A, Ds, y, ws, g, s);               \
        return 0;
    switch (g.R) {
        FD_SCAN_R(2) FD_SCAN_R(4) FD_SCAN_R(8) FD_SCAN_R(16) FD_SCAN_R(32)
    }
#undef FD_SCAN_R
    return -1;
}

template <typename T>
int dispatch_n(const T *xc, const float *xdbl, const float *dtw, const float *dtb, const float *A,
               const float *Ds, T *y, float *ws, const ScanGeom &g, hipStream_t s) {
    switch (g.N) {
    case 4: return dispatch_r<T, 4>(xc, xdbl, dtw, dtb, A, Ds, y, ws, g, s);
    case 8: return dispatch_r<T, 8>(xc, xdbl, dtw, dtb, A, Ds, y, ws, g, s);
    case 16: return dispatch_r<T, 16>(xc, xdbl, dtw, dtb, A, Ds, y, ws, g, s);
    case 32: return dispatch_r<T, 32>(xc, xdbl, dtw, dtb, A, Ds, y, ws, g, s);
    }
    return -1;
}

int chunk_len(int L, int D, bool low_latency) {
    // aim for >= ~4096 waves per image (4 per SIMD), chunk length a power of two in [32, 256] -- [64, 256] in the
    // throughput kernel set.  Deliberately independent of the batch size: a slice's result must not depend on what
    // else is in the batch (bitwise batch invariance -> sharding over GPUs changes nothing).
    // Round 4: 32-step chunks only pay for ONE slice (low_latency); from batch 8 up the chip is full anyway and a chunk
    // start costs its constants, its x_dbl staging and a carry entry: 64-step chunks measured 316 -> 270 us (d_inner 128,
    // N = 8 at 256x256) and 472 -> 429 us (d_inner 512, N = 16 at 128x128) at batch 8, level 0 (128 steps) unchanged.
    const int force = fd_dev(FD_DEV_SCAN_CL);     // development: chunk-length experiments
    if (force >= 32 && force <= 256 && (force & (force - 1)) == 0) return force;
    int64_t units = (int64_t)4 * (D / 64) * L;
    int cl = 256;
    const int cmin = low_latency ? 32 : 64;
    // (measured: 2048 / 1024 waves per image gain < 2 % at batch 8 and cost 8-30 % at batch 1)
    while (cl > cmin && units / cl < 4096) cl >>= 1;
    return cl;
}

ScanGeom make_geom(int B, int H, int W, int D, int N, int R, bool low_latency = false) {
    ScanGeom g;
    g.B = B; g.H = H; g.W = W; g.D = D; g.N = N; g.R = R; g.CD = R + 2 * N;
    g.H2 = (H + 1) / 2; g.W2 = (W + 1) / 2; g.L = g.H2 * g.W2;     // odd sizes: padded sub-grids (src/emamba2.py:191-199)
    g.CL = chunk_len(g.L, D, low_latency);
    g.nch = (g.L + g.CL - 1) / g.CL;
    g.xw = nullptr;
    g.xdbl_out = nullptr;
    g.low_latency = low_latency;
    return g;
}

}  // namespace

extern "C" int fd_selective_scan_fuses_xproj(int dtype, int D, int N, int R);

extern "C" int64_t fd_scan_ws_floats(int B, int H, int W, int D, int N) {
    ScanGeom g = make_geom(B, H, W, D, N, 1, true);        // the kernel set with the shorter chunks: an upper bound for both
    return 2 * (int64_t)B * 4 * g.nch * N * D;
}

// The shape checks of a scan call and its geometry: what scan_entry refuses, fd_selective_scan_geom refuses too.  g->xw is left
// NULL (the caller's pointer, or a placeholder for the query, goes there when `fused`).
static int scan_shape(int dtype_opts, bool fused, int B, int H, int W, int D, int N, int R, ScanGeom *g) {
    FD_REQUIRE(B > 0 && H > 0 && W > 0, "fd_selective_scan: bad batch / image size %d x %d x %d", B, H, W);
    FD_REQUIRE(D > 0 && D % 64 == 0, "fd_selective_scan: d_inner=%d must be a multiple of 64", D);
    FD_REQUIRE((int64_t)H * W * D * 4 < (1ll << 31), "fd_selective_scan: one image must stay below 2^31 bytes");
    FD_REQUIRE((N == 4 || N == 8 || N == 16 || N == 32) && (R == 2 || R == 4 || R == 8 || R == 16 || R == 32),
               "fd_selective_scan: unsupported d_state=%d / dt_rank=%d (need N in {4,8,16,32}, R in {2,4,8,16,32})", N, R);
    if (fused)
        FD_REQUIRE(fd_selective_scan_fuses_xproj(dtype_opts & (0xff | FD_OPT_F32_SPLIT), D, N, R), "fd_selective_scan_xproj: not available for this shape "
                   "(bf16 or fp32 | FD_OPT_F32_SPLIT, d_inner <= 256, (R + 2N) %% 4 == 0): D=%d N=%d R=%d", D, N, R);
    *g = make_geom(B, H, W, D, N, R, (dtype_opts & FD_OPT_LOW_LATENCY) != 0);
    return FD_OK;
}

// The chunk kernel's row buffer is held to 64 KiB.  Rows of N = 32 (68 floats with R <= 4, up to 96 with R = 32) in 256-step
// chunks (d_inner * L >= 2^24: beyond every size the model runs at, never launched by a test) would need 68-96 KiB.
static int scan_lds_ok(const ScanGeom &g, const ScanPlan &p) {
    FD_REQUIRE(p.seq || p.lds <= 65536, "fd_selective_scan: %d-step chunks of %d-float rows need %zu bytes of LDS (limit 65536): "
               "D=%d N=%d R=%d at %d x %d is not supported", g.CL, g.CD, p.lds, g.D, g.N, g.R, g.H, g.W);
    return FD_OK;
}

static int scan_entry(int dtype_opts, const void *xc, const void *x_proj_w, float *xdbl, const float *dtw, const float *dtb,
                      const float *A, const float *Ds, void *y, float *ws, int B, int H, int W, int D, int N, int R,
                      void *stream) {
    const int dtype = dtype_opts & 0xff;
    FD_REQUIRE(xc && xdbl && dtw && dtb && A && Ds && y && ws, "fd_selective_scan: null pointer");
    ScanGeom g;
    if (int rc = scan_shape(dtype_opts, x_proj_w != nullptr, B, H, W, D, N, R, &g)) return rc;
    if (x_proj_w) {
        FD_REQUIRE(((uintptr_t)x_proj_w & 15) == 0 && ((uintptr_t)xc & 15) == 0, "fd_selective_scan_xproj: 16-byte alignment");
        g.xw = x_proj_w;
        g.xdbl_out = xdbl;
    }
    if (int rc = scan_lds_ok(g, scan_plan(g, dtype == FD_BF16))) return rc;
    int rc = dtype == FD_BF16
                 ? dispatch_n<bf16>((const bf16 *)xc, xdbl, dtw, dtb, A, Ds, (bf16 *)y, ws, g, (hipStream_t)stream)
                 : dispatch_n<float>((const float *)xc, xdbl, dtw, dtb, A, Ds, (float *)y, ws, g, (hipStream_t)stream);
    FD_REQUIRE(rc == 0, "fd_selective_scan: unsupported d_state=%d / dt_rank=%d (need N in {4,8,16,32}, R in {2,4,8,16,32})", N, R);
    FD_LAUNCH_OK("fd_selective_scan");
    return FD_OK;
}

extern "C" int fd_selective_scan(int dtype, const void *xc, const float *xdbl, const float *dtw,
                                 const float *dtb, const float *A, const float *Ds, void *y, float *ws,
                                 int B, int H, int W, int D, int N, int R, void *stream) {
    return scan_entry(dtype, xc, nullptr, (float *)xdbl, dtw, dtb, A, Ds, y, ws, B, H, W, D, N, R, stream);
}

// 1 if fd_selective_scan_xproj can compute the x_proj rows inside its first phase for this shape: bf16, one
// workgroup per chunk (d_inner <= 256, so no workgroup repeats another's rows), rows of whole 16-byte groups.
extern "C" int fd_selective_scan_fuses_xproj(int dtype_opts, int D, int N, int R) {
    const int dtype = dtype_opts & 0xff;
    // (fp32 storage: only with FD_OPT_F32_SPLIT -- the x_proj rows then come from three bf16 MFMAs per product, which the exact
    //  fp32 parity mode does not use anywhere)
    // (measured, batch-8 launches of the fp32s forward, profiles/r06: d_inner 128 / N 4 at 512x512 1008 -> 953 us, d_inner 256 / N 8
    //  at 256x256 649 -> 630, d_inner 128 / N 8 at 256x256 355 -> 358; d_inner 256 / N 16 at 128x128 245 -> 267: the split costs
    //  VALU and registers in the phase that holds the widest state -- fused for N <= 8 only)
    const bool dt_ok = dtype == FD_BF16 || (dtype == FD_F32 && (dtype_opts & FD_OPT_F32_SPLIT) && N <= 8);
    return dt_ok && D % 64 == 0 && D <= 256 && (R + 2 * N) % 4 == 0;
}

// 1 if the engine should call fd_selective_scan_xproj for this block (x_proj inside the chunked scan's first phase),
// 0 if it should run the x_proj launch and fd_selective_scan: the single-pass scan of short sequences with a wide
// state takes its x_dbl rows from the workspace.  A function of the shape only.
extern "C" int fd_selective_scan_plan(int dtype_opts, int D, int N, int R, int H, int W) {
    const bool seq = !(dtype_opts & FD_OPT_LOW_LATENCY) && scan_seq_ok(H, W, D, N, R);
    return fd_selective_scan_fuses_xproj(dtype_opts & (0xff | FD_OPT_F32_SPLIT), D, N, R) && !seq;
}

// What a call of fd_selective_scan (fused = 0) / fd_selective_scan_xproj (fused = 1) with these arguments launches: scan_plan's
// answer, host only.  out is filled whenever the shape itself is valid, also when the call is refused for its LDS size.
extern "C" int fd_selective_scan_geom(int dtype_opts, int fused, int D, int N, int R, int H, int W, int32_t out[8]) {
    FD_REQUIRE(out, "fd_selective_scan_geom: null pointer");
    for (int i = 0; i < 8; ++i) out[i] = 0;
    ScanGeom g;
    if (int rc = scan_shape(dtype_opts, fused != 0, 1, H, W, D, N, R, &g)) return rc;
    if (fused) g.xw = out;                              // any non-NULL value: only tested, never read
    const ScanPlan p = scan_plan(g, (dtype_opts & 0xff) == FD_BF16);
    if (p.seq) return FD_OK;
    out[0] = 1;
    out[1] = g.CL;
    out[2] = g.nch;
    out[3] = p.two ? 2 : 1;
    out[4] = p.nw;
    out[5] = p.wgs;
    out[6] = p.carry;
    out[7] = (int32_t)p.lds;
    return scan_lds_ok(g, p);
}

extern "C" int fd_selective_scan_xproj(int dtype, const void *xc, const void *x_proj_w, float *xdbl, const float *dtw,
                                       const float *dtb, const float *A, const float *Ds, void *y, float *ws, int B,
                                       int H, int W, int D, int N, int R, void *stream) {
    FD_REQUIRE(x_proj_w, "fd_selective_scan_xproj: null x_proj weights");
    return scan_entry(dtype, xc, x_proj_w, xdbl, dtw, dtb, A, Ds, y, ws, B, H, W, D, N, R, stream);
}
