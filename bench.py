#!/usr/bin/env python3
"""Headline benchmark: denoised CT slices / second, 512x512, 50 DDIM steps, full FoundDiff
architecture (dim 64, mults 1-2-4-8, DA-CLIP RN50 conditioning), bf16 kernels, synthetic
weights + phantoms (BASELINE.json configs[2]; no checkpoints / Mayo data offline).

    python bench.py --gpus N --steps K --warmup W         (N>1: launched by torch.distributed.run)

A "step" = one complete sample() of a batch of `--batch` slices per GPU (DA-CLIP encode once,
50 UNet forwards + DDIM updates).  Slices are independent, so GPUs shard the slice range with
no data-path collective (weak scaling); one RCCL all-gather reassembles the output volume at
the end of the timed region.  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps and prints the line.  `--full` adds everything else the
benchmark measures, outside the timed region: the untimed replay under the rocm-smi clock / power sampler,
the H2D-inclusive repeat, the per-kernel roofline, the other precisions and samplers (fp16, fp32s, fp32,
fp8 25-step, ancestral, batch-1 latency) and the CPU baseline (each can still be switched off with its
--no-* option).  `--dump-outputs DIR` writes what the last timed step returned (see dump_outputs).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SIZE, S_DDIM = 512, 50
DIM, MULTS = 64, (1, 2, 4, 8)
PEAK_BF16_TFLOPS = 2500.0      # dense bf16 MFMA, MI355X_MICROARCH.md
PEAK_HBM_GBS = 8000.0          # HBM3E, MI355X_MICROARCH.md
ALG_GFLOP_PER_FORWARD = 575.5  # SURVEY.md section 8(d), 512x512, B=1


def build_model(device, size=SIZE, steps=S_DDIM, precision="bf16", seed=0):
    from founddiff_amd import arch, synth
    from founddiff_amd.DADiff import ResidualDiffusion, UnetRes, load_weights
    spec = arch.da_unet_spec(DIM, MULTS, prefix="model.unet0.")
    w = synth.synth_state_dict(spec, seed=seed)
    net = UnetRes(dim=DIM, dim_mults=MULTS, num_unet=1, condition=True, objective="pred_res",
                  test_res_or_noise="res", precision=precision)
    dif = ResidualDiffusion(net, image_size=size, timesteps=1000, sampling_timesteps=steps, objective="pred_res",
                            loss_type="l2", condition=True, sum_scale=0.01, test_res_or_noise="res")
    load_weights(dif, w, "synthetic weights")
    dif = dif.to(device)
    dif.init()
    return dif, w


def conv_flops(p):
    cin = p.c0 + p.c1
    if p.KH == 7 and cin == 8:
        cin = 2       # init_conv: channels 2..7 are zero padding, not algorithmic work
    fl = 2.0 * p.B * p.OH * p.OW * p.Cout * p.KH * p.KW * cin * p.ndir
    if p.prologue == 3:      # PRO_LN_GATE_ZRE: the z half of in_proj (Cout -> Cin) runs inside out_proj
        fl += 2.0 * p.B * p.OH * p.OW * p.Cout * cin
    return fl


def _time_launches(lib, launches, reps=5):
    """Best-of-`reps` HIP-event time (ms) of replaying `launches` back to back.  Every launch of this
    library goes to torch's CURRENT stream (engine.stream), which is the stream torch.cuda.Event
    records on."""
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        ev0.record()
        for n, a in launches:
            getattr(lib, n)(*a)
        ev1.record()
        ev1.synchronize()
        ms = ev0.elapsed_time(ev1)
        best = ms if best is None else min(best, ms)
    return best


def csrc_sha():
    """hash of the kernel sources: profiles/traffic.json records the one it was measured with"""
    import glob
    import hashlib
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "founddiff_amd", "csrc", "*"))):
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


TRANSCENDENTALS_PER_S = 256 * 4 * 8 * 2.4e9       # v_exp / v_log: 8 lanes per clock per SIMD (MI355X_MICROARCH.md, issue cost 8 cyc)
HBM_ACHIEVABLE_BPS = 6.3e12                       # MI355X_MICROARCH.md: 6.29 TB/s measured copy rate


def forward_bounds(eng, H, W, traffic, t_measured_ms):
    """Whole-forward bounds per slice (ms): HBM at the achievable rate over the measured traffic, the bf16 MFMA peak
    over the algorithmic FLOPs, and the transcendental-issue floor of the selective scans ((N + 2) v_exp / v_log per
    channel and position and pass: the chunked form runs two passes, the single-pass form of short sequences one)."""
    from founddiff_amd import _lib as L
    lib = L.lib()
    levels = []
    h, w = H, W
    for d in eng.downs:
        levels.append((d["mamba"], h, w))
        if d["stride"] == 2:
            h, w = h // 2, w // 2
    levels.append((eng.mid_mamba, h, w))
    for u in eng.ups:
        levels.append((u["mamba"], h, w))
        if u["up"]:
            h, w = 2 * h, 2 * w
    ntr = 0.0
    for m, hh, ww in levels:
        fused = lib.fd_selective_scan_plan(getattr(eng, "scan_dt", eng.dt), m["D"], m["N"], m["R"], hh, ww)
        single = (not fused) and m["N"] >= 16 and ((hh + 1) // 2) * ((ww + 1) // 2) <= 1024 and m["R"] % 8 == 0 and not eng.low_latency
        ntr += 4.0 * m["D"] * ((hh + 1) // 2) * ((ww + 1) // 2) * (m["N"] + 2) * (1 if single else 2)
    tot = traffic.get("total_hbm_bytes_per_forward")
    nb = traffic.get("batch", 8)
    out = {"t_measured": round(t_measured_ms, 4),
           "t_mfma": round(ALG_GFLOP_PER_FORWARD * 1e9 / (PEAK_BF16_TFLOPS * 1e12) * 1e3, 4),
           "t_scan_transcendental_floor": round(ntr / TRANSCENDENTALS_PER_S * 1e3, 4),
           "scan_transcendentals": int(ntr), "unit": "ms per slice-forward"}
    if tot:
        out["hbm_bytes_measured"] = int(tot / nb)
        out["t_hbm_at_6.3TBps"] = round(tot / nb / HBM_ACHIEVABLE_BPS * 1e3, 4)
        out["traffic_measured_with_current_kernels"] = traffic.get("csrc_sha") == csrc_sha()
        out["frac_of_bound"] = round(max(out["t_hbm_at_6.3TBps"], out["t_mfma"], out["t_scan_transcendental_floor"]) / t_measured_ms, 3)
    return out


def roofline_leg(dif, x, noise, t_measured_ms=None, clock_replay=True):
    """Roofline of the dominant kernel symbol of one UNet forward -- the symbol with the largest total time, which is
    also the top symbol of the rocprofv3 --stats summary of this command (profiles/).  Candidates: pwdw_kernel<64|128,false>, pwdw_kernel<64,true> and
    pwdw_gram_kernel (fused LayerNorm+modulate -> 1x1 -> depthwise 3x3 [-> Gram | -> project_out] of the 64- / 128-channel Mamba
    blocks: HBM roofline), gemm_rows_zre_kernel (out_proj with the z gate recomputed: HBM), down_fused_kernel (GroupNorm apply + 4x4 / stride-2 convolution: HBM), the two instantiations of conv3x3_halo_kernel (MFMA roofline) and dwconv3x3_bf16_kernel (HBM).  Each is
    measured by replaying exactly its launches of one forward between HIP events on the launch stream; the largest
    becomes `roofline`, the rest `roofline.others`.  `forward`: the whole-forward bounds (forward_bounds)."""
    from founddiff_amd import _lib as L
    eng = dif._eng()
    # the timed region launches every kernel on sub-batches (concurrent half-batches): measure that launch shape
    if x.shape[0] >= 8 and x.shape[0] % dif.streams == 0:
        x, noise = x[:x.shape[0] // dif.streams], noise[:x.shape[0] // dif.streams]
    B = x.shape[0]
    x_in = (x * 2 - 1).contiguous()
    img = (x_in + 0.1 * noise).contiguous()
    tb = torch.full((B,), 500.0, device=x.device)
    eng.encode_condition(x_in)
    eng.forward(img, x_in, tb)
    L.TRACE = []
    eng.forward(img, x_in, tb)
    trace, L.TRACE = L.TRACE, None
    lib = L.lib()
    traffic = {}
    tp = os.path.join(ROOT, "profiles", "traffic.json")
    if os.path.exists(tp):
        traffic = json.load(open(tp))
    all_ms = _time_launches(lib, trace, reps=2)
    esz = 2                                                     # bf16

    def hbm_entry(kernel, launches, nbytes, key):
        ms = _time_launches(lib, launches)
        gbs = nbytes / (ms * 1e-3) / 1e9
        return {"bound": "hbm", "kernel": kernel, "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                "frac": round(gbs / PEAK_HBM_GBS, 4), "traffic": traffic.get(key),
                "launches_per_forward": len(launches), "avg_launch_us": round(ms * 1e3 / len(launches), 2),
                "alg_bytes_per_launch": round(nbytes / len(launches)), "kernel_ms_per_forward": round(ms, 3)}

    cands, scan_entries = [], []
    # fused 1x1 -> depthwise.  args = (dtype, x, ld_x, off_x, Cin, gamma, beta, eps, shift, scale, ln_ld,
    #      w_pw, Cdw, w_dw, b_dw, silu, out_dw, ld_dw, off_dw, Cz, out_z, ld_z, off_z, B, H, W, stream)
    # (two symbols: pwdw_kernel<64> serves the 64-channel blocks, <128> the C = 128 block at 256x256)
    for cin in (64, 128):
        pw = [(n, a) for n, a in trace if n == "fd_pw_dw3x3" and a[4] == cin]
        if pw:
            pw_bytes = sum(1.0 * a[23] * a[24] * a[25] * (a[4] + a[12] + a[19]) * esz for _, a in pw)   # in + dw out + z out, once
            cands.append(hbm_entry("pwdw_kernel<%d,false>" % cin, pw, pw_bytes, "pwdw%d_hbm_bytes_per_launch" % cin))
    # the v branch of the channel attention through project_out (pwdw_kernel<64,true>): args = (dtype, x, ld_x, off_x, Cin, gamma,
    #      beta, eps, shift, scale, ln_ld, w_pw, w_dw, w2, gate, gate_ld, out, ld_o, off_o, B, H, W, stream): 64 channels in, 64 out
    pj = [(n, a) for n, a in trace if n == "fd_pw_dw3x3_proj"]
    if pj:
        pj_bytes = sum(1.0 * a[19] * a[20] * a[21] * (64 + 64) * esz for _, a in pj)
        cands.append(hbm_entry("pwdw_kernel<64,true>", pj, pj_bytes, "pwdw_proj_hbm_bytes_per_launch"))
    # GroupNorm apply + 4x4 / stride-2 convolution in one pass (down_fused_kernel): args = (dtype, h, x, mean_rstd, gamma, beta,
    #      groups, skip, w, bias, out, B, H, W, C, Cout, stream): h and x in, skip and the down-sampled tensor out, once
    dn = [(n, a) for n, a in trace if n == "fd_gn_apply_down4x4"]
    if dn:
        dn_bytes = sum(1.0 * a[11] * a[12] * a[13] * (3 * a[14] + a[15] / 4.0) * esz for _, a in dn)
        cands.append(hbm_entry("down_fused_kernel", dn, dn_bytes, "down_fused_hbm_bytes_per_launch"))
    # out_proj with the z gate recomputed (gemm_rows_zre_kernel): y (K) + block input (Cout) in, Cout out, once
    zr = [(n, a) for n, a in trace if n == "fd_conv2d" and a[0]._obj.prologue == 3]
    if zr:
        zr_bytes = sum(1.0 * a[0]._obj.B * a[0]._obj.H * a[0]._obj.W * (a[0]._obj.c0 + 2 * a[0]._obj.Cout) * esz for _, a in zr)
        cands.append(hbm_entry("gemm_rows_zre_kernel", zr, zr_bytes, "gemm_rows_zre_hbm_bytes_per_launch"))
    # ... with the Gram: args = (dtype, x, ld_x, off_x, Cin, gamma, beta, eps, shift, scale, ln_ld, w_pw, w_dw, out_v, ld_v,
    #      off_v, partial, B, H, W, stream): reads 64 channels, writes v (64 channels) + one Gram partial per workgroup
    pg = [(n, a) for n, a in trace if n == "fd_pw_dw3x3_gram"]
    if pg:
        has_v = lambda a: bool(getattr(a[13], "value", a[13]))        # out_v == NULL: q, k only (v recomputed by fd_pw_dw3x3_proj)
        pg_bytes = sum(1.0 * a[17] * a[18] * a[19] * (64 + (64 if has_v(a) else 0)) * esz
                       + 1.0 * a[17] * 2 * lib.fd_pw_dw3x3_gram_nblk_opts(a[0], a[18], a[19]) * 1088 * 4 for _, a in pg)
        cands.append(hbm_entry("pwdw_gram_kernel", pg, pg_bytes, "pwdw_gram_hbm_bytes_per_launch"))
    # the two instantiations of the halo 3x3 kernel separately (separate symbols in the rocprof summary: <128,8> serves
    # Cout > 64, <64,16> / <64,8> Cout <= 64)
    halo = [(n, a) for n, a in trace if n == "fd_conv2d" and lib.fd_conv_kernel_id(a[0]) == 11]
    for name, sel, tkey in (("conv3x3_halo_kernel<128,8,false>", lambda q: q.Cout > 64, "conv3x3_halo128_hbm_bytes_per_launch"),
                            ("conv3x3_halo_kernel<64,16|8,false>", lambda q: q.Cout <= 64, "conv3x3_halo64_hbm_bytes_per_launch")):
        part = [(n, a) for n, a in halo if sel(a[0]._obj)]
        if not part:
            continue
        fl = sum(conv_flops(a[0]._obj) for _, a in part)
        ms = _time_launches(lib, part)
        tf = fl / (ms * 1e-3) / 1e12
        cands.append({"bound": "mfma", "kernel": name, "achieved": round(tf, 1),
                      "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(tf / PEAK_BF16_TFLOPS, 4),
                      "traffic": traffic.get(tkey, traffic.get("conv3x3_halo_hbm_bytes_per_launch")),     # (per symbol; the family figure as fallback)
                      "launches_per_forward": len(part), "avg_launch_us": round(ms * 1e3 / len(part), 2),
                      "alg_gflop_per_launch": round(fl / 1e9 / len(part), 2),
                      "kernel_ms_per_forward": round(ms, 3)})
    # the up-sampling 3x3 convolutions as four 2x2 convolutions on the source grid (conv3x3_halo_kernel<..., UP>, kernel id 14):
    # priced with the FLOPs the kernel EXECUTES (4 taps per output; the reference's 9-tap form of the same sums is 2.25 x that)
    up = [(n, a) for n, a in trace if n == "fd_conv2d" and lib.fd_conv_kernel_id(a[0]) == 14]
    if up:
        fl9 = sum(conv_flops(a[0]._obj) for _, a in up)
        fl = fl9 * 4.0 / 9.0
        ms = _time_launches(lib, up)
        tf = fl / (ms * 1e-3) / 1e12
        cands.append({"bound": "mfma", "kernel": "conv3x3_halo_kernel<128|64,8|16,false,UP> (up-sampling 3x3 as four 2x2 on the source grid)",
                      "achieved": round(tf, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(tf / PEAK_BF16_TFLOPS, 4),
                      "traffic": traffic.get("conv3x3_up_hbm_bytes_per_launch"), "launches_per_forward": len(up),
                      "avg_launch_us": round(ms * 1e3 / len(up), 2), "alg_gflop_per_launch": round(fl / 1e9 / len(up), 2),
                      "gflop_per_launch_of_the_9_tap_form": round(fl9 / 1e9 / len(up), 2), "kernel_ms_per_forward": round(ms, 3)})
    # 3x3 64 -> 64 with the weights resident in registers (conv3x3_rw_kernel): MFMA roofline like the halo kernel
    rw = [(n, a) for n, a in trace if n == "fd_conv2d" and lib.fd_conv_kernel_id(a[0]) == 13]
    if rw:
        fl = sum(conv_flops(a[0]._obj) for _, a in rw)
        ms = _time_launches(lib, rw)
        tf = fl / (ms * 1e-3) / 1e12
        cands.append({"bound": "mfma", "kernel": "conv3x3_rw_kernel", "achieved": round(tf, 1), "peak": PEAK_BF16_TFLOPS,
                      "unit": "TFLOP/s", "frac": round(tf / PEAK_BF16_TFLOPS, 4), "traffic": traffic.get("conv3x3_rw_hbm_bytes_per_launch"),
                      "launches_per_forward": len(rw), "avg_launch_us": round(ms * 1e3 / len(rw), 2),
                      "alg_gflop_per_launch": round(fl / 1e9 / len(rw), 2), "kernel_ms_per_forward": round(ms, 3)})
    # depthwise 3x3 alone: args = (dtype, in, ld_in, off_in, w, bias, silu, out, ld_out, off_out, B, H, W, C, stream)
    dws = [(n, a) for n, a in trace if n == "fd_dwconv3x3"]
    if dws:
        dw_bytes = sum(2.0 * a[10] * a[11] * a[12] * a[13] * esz for _, a in dws)
        cands.append(hbm_entry("dwconv3x3_bf16_kernel", dws, dw_bytes, "dwconv3x3_bf16_hbm_bytes_per_launch"))
    # selective scans (the largest kernel family of the forward): one entry per symbol group, each against TWO bounds -- HBM
    # (u once + y once + the x_dbl rows once) and the transcendental-issue floor ((N + 2) v_exp / v_log per channel, position
    # and PASS: two passes in the chunked form, one in the single-pass form); `frac` is taken against the tighter (larger) one.
    # fd_selective_scan_xproj args = (dtype, u, x_proj, x_dbl, dt_w, dt_b, A, D, y, ws, B, H, W, d_inner, N, R, stream);
    # fd_selective_scan       args = (dtype, u, x_dbl, dt_w, dt_b, A, D, y, ws, B, H, W, d_inner, N, R, stream)
    def scan_geom(n, a):
        o = 10 if n == "fd_selective_scan_xproj" else 9
        return a[o], a[o + 1], a[o + 2], a[o + 3], a[o + 4], a[o + 5]
    scans = [(n, a) for n, a in trace if n in ("fd_selective_scan_xproj", "fd_selective_scan")]
    groups = {}
    for n, a in scans:
        b_, h_, w_, d_, n_, r_ = scan_geom(n, a)
        lq = ((h_ + 1) // 2) * ((w_ + 1) // 2)
        single = n == "fd_selective_scan" and n_ >= 16 and lq <= 1024 and r_ % 8 == 0 and not eng.low_latency
        if single:
            key = "scan_seq_kernel (single pass, N >= 16, L <= 1024)"
        elif d_ == 128 and n_ <= 4:
            key = "scan_chunk_kernel x2 + scan_carry_kernel, level 0 (d_inner 128, N 4, two channels per lane)"
        else:
            key = "scan_chunk_kernel x2 + scan_carry_kernel, levels 1-2 (N 8..16)"
        groups.setdefault(key, []).append((n, a, single))
    for key, part in groups.items():
        launches = [(n, a) for n, a, _ in part]
        nbytes = ntr = 0.0
        for n, a, single in part:
            b_, h_, w_, d_, n_, r_ = scan_geom(n, a)
            lq = ((h_ + 1) // 2) * ((w_ + 1) // 2)
            nbytes += 2.0 * b_ * 4 * lq * d_ * esz + 1.0 * b_ * 4 * lq * (r_ + 2 * n_) * 4
            ntr += 1.0 * b_ * 4 * lq * d_ * (n_ + 2) * (1 if single else 2)
        ms = _time_launches(lib, launches)
        t_hbm, t_tr = nbytes / (PEAK_HBM_GBS * 1e9) * 1e3, ntr / TRANSCENDENTALS_PER_S * 1e3
        gbs = nbytes / (ms * 1e-3) / 1e9
        ent = {"bound": "hbm" if t_hbm >= t_tr else "transcendental issue (v_exp / v_log at 8 lanes per clock per SIMD)",
               "kernel": key, "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
               "frac_hbm": round(t_hbm / ms, 4), "frac_transcendental": round(t_tr / ms, 4), "frac": round(max(t_hbm, t_tr) / ms, 4),
               "t_hbm_bound_ms": round(t_hbm, 4), "t_transcendental_floor_ms": round(t_tr, 4),
               "traffic": traffic.get("scan_hbm_bytes_per_launch", {}).get(key.split(",")[0] + ("|l0" if "level 0" in key else "|l12" if "levels 1-2" in key else ""))
               if isinstance(traffic.get("scan_hbm_bytes_per_launch"), dict) else None,
               "launches_per_forward": len(launches), "avg_launch_us": round(ms * 1e3 / len(launches), 2),
               "alg_bytes_per_launch": round(nbytes / len(launches)), "kernel_ms_per_forward": round(ms, 3)}
        scan_entries.append(ent)
    # (~1.5 s of halo-conv launches next to a rocm-smi call; skipped under rocprofv3, whose --stats would count them)
    box = clocks_under_load(lib, halo) if clock_replay else None
    # the headline `roofline` = the entry with the largest time per forward over symbol GROUPS (round 6): a scan group (two
    # chunked phases + the carry kernel, or the single-pass kernel) competes with the convolution / fused-kernel symbols, so the
    # scan is the headline while it is the largest consumer.  Its `frac` is taken against the tighter of its two bounds (`bound`
    # names it; `frac_hbm` / `frac_transcendental` carry both).
    scan_entries.sort(key=lambda c: -c["kernel_ms_per_forward"])
    allc = sorted(cands + scan_entries, key=lambda c: -c["kernel_ms_per_forward"])
    res = dict(allc[0])
    res["box_under_halo_replay"] = box
    short = {"level 0": "scan_level0", "levels 1-2": "scan_levels12", "single pass": "scan_seq"}
    for c in scan_entries:          # ... and every scan group at the top level of `roofline`, next to `forward`
        for pat, key in short.items():
            if pat in c["kernel"]:
                res[key] = c
    res.update({"all_kernels_ms_per_forward": round(all_ms, 3), "batch": B, "others": allc[1:],
                "scan_family_ms_per_forward": round(sum(c["kernel_ms_per_forward"] for c in scan_entries), 3),
                "forward": forward_bounds(eng, x.shape[2], x.shape[3], traffic, t_measured_ms if t_measured_ms else all_ms / B),
                "note": "every kernel replayed ALONE on the launch stream at the sub-batch the timed region launches (8): the "
                        "figures a kernel reaches when it owns the chip.  In the timed region two sub-batches run on two "
                        "streams, so rocprofv3's per-kernel durations of the default command include co-scheduling; the "
                        "summary of `FOUNDDIFF_STREAMS=1 python bench.py --batch 8` (profiles/) is the one whose averages "
                        "agree with avg_launch_us"})
    return res


def cpu_baseline_leg(w, x_in01, noise, n_forwards=3):
    """CPU oracle (PyTorch-CPU + C/OpenMP scan) on the host cores: DA-CLIP encode + `n_forwards` of the 50
    UNet forwards of one 512x512 slice (three different timesteps), extrapolated to 50 (BASELINE.md section 3:
    >= 3 steps at config 3)."""
    from oracle import nets, sampler
    # 32 threads: on the 256-core GPU box PyTorch-CPU is SLOWER with all cores (oversubscribed
    # intra-op pools: 134 s for the same sample at 256 threads); `cores` reports what was used
    nthr = min(32, os.cpu_count())
    torch.set_num_threads(nthr)
    os.environ["OMP_NUM_THREADS"] = str(nthr)
    orc = sampler.ResidualOracle(w, prefix="model.unet0.", sampling_timesteps=S_DDIM)
    xi = x_in01[:1].cpu() * 2 - 1
    xt = xi + 0.1 * noise[:1].cpu()
    t0 = time.time()
    orc._cond = nets.da_unet_cond(orc.sd, xi)
    t1 = time.time()
    per_fwd = []
    for t in (999, 499, 19)[:n_forwards]:
        ts = time.time()
        orc.unet(xt, xi, torch.full((1,), t, dtype=torch.long))
        per_fwd.append(time.time() - ts)
    fwd = sum(per_fwd) / len(per_fwd)
    per_slice = (t1 - t0) + S_DDIM * fwd
    # why 32 threads: one more forward each at other TORCH intra-op thread counts (s per forward), reported, not used
    # for `value`.  Only torch's pool changes: the C/OpenMP scan oracle's runtime is initialised by then and keeps the
    # thread count it started with (nthr) -- the sweep is labelled accordingly.
    sweep = {str(nthr): round(fwd, 2)}
    for n in (8, 16, 64, 128):
        if n != nthr and n <= os.cpu_count():
            torch.set_num_threads(n)
            ts = time.time()
            orc.unet(xt, xi, torch.full((1,), 499, dtype=torch.long))
            sweep[str(n)] = round(time.time() - ts, 2)
    torch.set_num_threads(nthr)
    return {"value": round(1.0 / per_slice, 6), "unit": "slices/s", "cores": nthr, "kind": "port",
            "sample": f"1 slice: DA-CLIP encode ({t1 - t0:.1f}s) + {len(per_fwd)} of {S_DDIM} UNet forwards "
                      f"({', '.join('%.1f' % v for v in per_fwd)} s) at 512x512 fp32, extrapolated to {S_DDIM}",
            "seconds_per_forward_by_torch_threads": sweep, "host_cores": os.cpu_count()}


def fp32_parity_leg(dev, x, noise, steps=1, precision="fp32"):
    """Throughput of a parity-grade mode (the modes that carry the 1e-3 gate against the CPU reference) on the same
    workload, outside the timed region: `steps` complete 50-step sample() calls of the same batch.  'fp32': fp32 storage,
    exact-f32 MFMA.  'fp32s': fp32 storage, every contraction as three bf16 MFMAs on hi / lo operand halves (4.4e-6 per
    contraction against the exact form); tests/test_gpu_round5.py holds its whole loop to the same 1e-3."""
    dif, _ = build_model(dev, precision=precision)
    B = x.shape[0]
    dif.sample([x], batch_size=B, noise=noise)          # warm-up: workspaces + graph capture
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        dif.sample([x], batch_size=B, noise=noise)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    del dif
    torch.cuda.empty_cache()
    return {"value": round(B / dt, 4), "unit": "slices/s", "ms_per_step": round(dt * 1e3, 2),
            "ms_per_unet_forward_per_slice": round(dt / S_DDIM / B * 1e3, 3), "steps": steps, "batch": B,
            "dtype": {"fp32": "f32 storage, exact-f32 MFMA", "fp32s": "f32 storage, split-bf16 contractions (3 bf16 MFMAs per product)",
                      "fp16": "the bf16 engine's kernels on the library's IEEE-binary16 build (libfounddiff_hip_f16.so): f16 storage "
                              "and MFMA operands, f32 accumulation; whole last step on the fp32s engine"}[precision],
            "gate": ("<= 1e-3 L2 (>= 70 dB) vs the CPU oracle over the 50-step loop at 256x256 and 512x512 on the tests' model, measured "
                     "6.9e-4 / 6.3e-4, max-rel 1.5e-3 (tests/test_gpu_fp16.py); 6.7e-4 .. 1.7e-3 over four random-weight models, 6-13x "
                     "below bf16 on each; binary16 range: a non-finite result raises" if precision == "fp16" else
                     "<= 1e-3 max-rel vs the reference goldens and the CPU oracle (tests/test_gpu_e2e.py, tests/test_gpu_round5.py)")}


def fp8_leg(dev, x, noise, ddim_steps=25):
    """BASELINE configs[4] geometry outside the timed region: e4m3 weights + e4m3 halo on the fp8 MFMA in the eligible
    3x3 convolutions, 25-step DDIM, same batch -- so that the driver's record carries the number."""
    dif, _ = build_model(dev, steps=ddim_steps, precision="fp8")
    B = x.shape[0]
    dif.sample([x], batch_size=B, noise=noise)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dif.sample([x], batch_size=B, noise=noise)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del dif
    torch.cuda.empty_cache()
    return {"value": round(B / dt, 4), "unit": "slices/s", "ddim_steps": ddim_steps, "batch": B,
            "ms_per_unet_forward_per_slice": round(dt / ddim_steps / B * 1e3, 3),
            "dtype": "bf16 activations, e4m3 weights (fp8 MFMA) in the 3x3 convs; last step's levels 0-1 on the bf16 engine",
            "workload": "BASELINE configs[4] geometry: 512x512, 25-step DDIM (single GPU, synthetic mixed-dose phantoms)"}


def ancestral_leg(dev, x, chunks=2):
    """BASELINE configs[3]'s sampler (1000-step ancestral p_sample_loop, per-slice keyed step noise) outside the timed
    region: `chunks` replays of the captured step chunk + the tail step are TIMED, the 1000-step figure is an
    EXTRAPOLATION from them (a full volume takes ~30 s per 16 slices; `--sampler ancestral` times it for real)."""
    dif, _ = build_model(dev, steps=1000)
    B = x.shape[0]
    seeds = torch.arange(B, dtype=torch.int64) + 5000
    dif._anc_max_chunks = 1
    dif.sample([x], batch_size=B, slice_seeds=seeds)                    # warm-up: graph capture
    dif._anc_max_chunks = chunks
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dif.sample([x], batch_size=B, slice_seeds=seeds)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    nsteps = dif._anc_steps_run
    del dif
    torch.cuda.empty_cache()
    per_step = dt / nsteps
    return {"value": round(B / (per_step * 1000), 5), "unit": "slices/s", "extrapolated": True,
            "timed": f"{nsteps} of 1000 steps ({chunks} graph chunks + the tail step) incl. the DA-CLIP encode, batch {B}",
            "ms_per_step_per_slice": round(per_step / B * 1e3, 4),
            "workload": "BASELINE configs[3] sampler: 512x512, 1000-step ancestral, keyed per-slice step noise (one GPU's share)"}


def latency_leg(dev, x, noise, reps=3):
    """The reference's own evaluation shape (Trainer.test is batch 1, /root/reference/src/DADiff.py:1823-1868) outside the
    timed region: ONE 512x512 slice, 50-step DDIM, the `low_latency` kernel set (chunked scans at every level), whole
    loop as one HIP graph.  ms per denoised slice, DA-CLIP encode included."""
    dif, _ = build_model(dev)
    dif.model.unet0.low_latency = True
    x1, n1 = x[:1].contiguous(), noise[:1].contiguous()
    dif.sample([x1], batch_size=1, noise=n1)            # warm-up: workspaces + loop-graph capture
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        dif.sample([x1], batch_size=1, noise=n1)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    del dif
    torch.cuda.empty_cache()
    best = min(ts)
    return {"value": round(best * 1e3, 2), "unit": "ms per 50-step slice", "batch": 1, "reps": reps,
            "ms_per_unet_forward": round(best / S_DDIM * 1e3, 3), "slices_per_s": round(1.0 / best, 3),
            "kernel_set": "low_latency (Trainer.test(batch_size=1))", "higher_is_better": False}


def _smi_read():
    """(sclk MHz, mclk MHz, socket power W) from one rocm-smi call, None where not available"""
    import re
    import subprocess
    r = subprocess.run(["rocm-smi", "--showclocks", "--showpower", "--showmaxpower", "--json"], capture_output=True, text=True, timeout=30)
    d = json.loads(r.stdout)
    card = d.get("card0") or next(iter(d.values()))
    out = {}
    for k, v in card.items():
        kl = k.lower()
        m = re.search(r"([0-9.]+)", str(v))
        if not m:
            continue
        if kl.startswith("sclk") and "level" not in kl:
            out["sclk_mhz"] = float(m.group(1))
        elif kl.startswith("mclk") and "level" not in kl:
            out["mclk_mhz"] = float(m.group(1))
        elif "max" in kl and "power" in kl:
            out["power_cap_w"] = float(m.group(1))
        elif "power" in kl and "(w)" in kl:
            out["socket_power_w"] = float(m.group(1))
    return out


class SmiSampler:
    """Polls rocm-smi from a host thread while the timed region runs: mean / min shader clock and mean socket power of
    the region.  The headline workload holds the socket at its power cap (~1.4 kW) with the shader clock near 2.0 GHz
    instead of the 2.4 GHz the peaks are quoted at: the reading says how much of a box-to-box difference is clock."""

    def __init__(self, period=0.4):
        import threading
        self.period, self.samples, self._stop = period, [], threading.Event()
        self._thr = threading.Thread(target=self._run, daemon=True)

    def _run(self):
        while not self._stop.is_set():
            try:
                self.samples.append(_smi_read())
            except Exception:                               # noqa: BLE001 -- a reading, not a requirement
                pass
            self._stop.wait(self.period)

    def __enter__(self):
        self._thr.start()
        return self

    def __exit__(self, *a):
        self._stop.set()
        self._thr.join(timeout=40)

    def summary(self):
        sc = [q["sclk_mhz"] for q in self.samples if "sclk_mhz" in q]
        pw = [q["socket_power_w"] for q in self.samples if "socket_power_w" in q]
        if not sc:
            return None
        cap = [q["power_cap_w"] for q in self.samples if "power_cap_w" in q]
        return {"samples": len(sc), "sclk_mhz_mean": round(sum(sc) / len(sc), 1), "sclk_mhz_min": min(sc),
                "socket_power_w_mean": round(sum(pw) / len(pw), 1) if pw else None, "power_cap_w": cap[0] if cap else None}


def clocks_under_load(lib, launches, seconds=1.5):
    """Shader clock and socket power WHILE the halo-conv launches replay (rocm-smi next to ~1.5 s of queued kernels), so a
    bench line can be attributed to its box: the pool's boxes differ by up to 1.5x on the MFMA-bound kernels
    (profiles/README.md).  None where rocm-smi is not usable."""
    if not launches:
        return None
    one = _time_launches(lib, launches, reps=1)
    n = max(1, min(4000, int(seconds * 1e3 / max(one, 1e-3))))
    for _ in range(n):
        for name, args in launches:
            getattr(lib, name)(*args)
    out = None
    try:
        out = _smi_read()
        out["queued_ms"] = round(one * n, 1)
    except Exception as e:                               # noqa: BLE001 -- a reading, not a requirement
        out = {"error": f"{type(e).__name__}: {e}"[:200]}
    torch.cuda.synchronize()
    return out


DUMP_CAP_BYTES = 64 << 20


def dump_outputs(out_dir, arrays, cap=DUMP_CAP_BYTES):
    """Write {name: tensor} as out_dir/<name>.npy in float32.  Each array gets an equal share of `cap`; one over its share
    is cut to a fixed sample of its slices along dim 0 (seeded, sorted indices: the same ones from run to run for the
    same arguments)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    share = cap // max(1, len(arrays))
    for name, t in arrays.items():
        a = t.detach().float().cpu().numpy()
        if a.nbytes > share:
            per = a.nbytes // a.shape[0]
            idx = np.sort(np.random.default_rng(0).choice(a.shape[0], max(1, share // per), replace=False))
            a = a[idx]
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a))


def self_launch(a):
    """`python bench.py --gpus N` from a bare shell: start the N ranks as a CHILD torch.distributed.run (this
    process never touches a GPU), relay its output and exit with its code."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    raise SystemExit(subprocess.run(cmd, env=env).returncode)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=16, help="slices per GPU per step (run as two concurrent half-batches)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the outputs of the last timed step as DIR/<name>.npy (float32, "
                    "<= 64 MB in all): `denoised` = sample()[-1] (the volume), `noisy_input` = sample()[0]")
    ap.add_argument("--full", action="store_true", help="also run the measurements beyond the headline figure (clock / power "
                    "sampler, H2D-inclusive repeat, roofline, other precisions and samplers, CPU baseline); the --no-* "
                    "options below switch parts of it off")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-clock-replay", action="store_true", help="skip the 1.5 s halo-conv replay behind "
                    "roofline.box_under_halo_replay (for runs under rocprofv3 --stats: the replayed launches would be counted)")
    ap.add_argument("--no-fp32-leg", action="store_true")
    ap.add_argument("--no-smi", action="store_true", help="skip the untimed replay with the rocm-smi clock / power sampler")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp8", "fp16"],
                    help="fp8: BASELINE configs[4] -- e4m3 weights on the fp8 MFMA for the 3x3 convs; fp16: the same kernels on the "
                         "library's binary16 build; separate variants, never the headline")
    ap.add_argument("--ddim-steps", type=int, default=S_DDIM, help="25 with --precision fp8 reproduces configs[4]")
    ap.add_argument("--sampler", default="ddim", choices=["ddim", "ancestral"],
                    help="ancestral: BASELINE configs[3]'s 1000-step p_sample_loop (keyed per-slice step noise) as the timed "
                         "workload -- ~30 s per step of 16 slices; a separate variant, never the headline")
    ap.add_argument("--no-extra-legs", action="store_true", help="skip the fp8 (configs[4]) and ancestral (configs[3]) legs")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if a.sampler == "ancestral":
        a.ddim_steps = 1000

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if "RANK" not in os.environ and (a.gpus > 1 or os.environ.get("FOUNDDIFF_BENCH_FORCE_LAUNCH") == "1"):
        self_launch(a)
    if a.gpus > 1 and world != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {a.gpus}")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=dev)

    from founddiff_amd import parallel, synth
    dif, w = build_model(dev, steps=a.ddim_steps, precision=a.precision)
    B = a.batch
    # global slice range sharded contiguously over ranks; per-slice noise keyed by GLOBAL index
    lo, hi = parallel.shard_range(world * B, world, rank)
    _, ld = synth.ct_phantom(world * B, SIZE, seed=10)
    x = torch.from_numpy(ld[lo:hi]).to(dev)
    noise = torch.stack([torch.randn(1, SIZE, SIZE, generator=torch.Generator().manual_seed(1000 + i))
                         for i in range(lo, hi)]).to(dev)

    seeds = torch.arange(lo, hi, dtype=torch.int64) + 1000      # ancestral: step noise keyed by the GLOBAL slice index

    def step():
        outs = dif.sample([x], batch_size=B, noise=noise, slice_seeds=seeds)
        return outs, parallel.gather_volume(outs[-1], world)

    for _ in range(a.warmup):
        step()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        outs, vol = step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    if a.dump_outputs:
        noisy = parallel.gather_volume(outs[0], world)          # (a collective: every rank takes part, rank 0 writes)
        if rank == 0:
            dump_outputs(a.dump_outputs, {"denoised": vol, "noisy_input": noisy})
    # shader clock / socket power of this workload on this box: sampled over an identical UNTIMED replay of the timed region
    # (rocm-smi forked every 0.4 s from a host thread: host contention and SMU queries stay out of the headline number)
    smi = None
    if a.full and not a.no_smi and world == 1:     # (single-GPU runs only: the multi-rank path stays exactly the timed region + its reduction)
        smi = SmiSampler()
        smi.__enter__()
        for _ in range(max(1, min(a.steps, 3))):
            step()
        torch.cuda.synchronize()
        smi.__exit__()
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    assert vol.shape[0] == world * B and torch.isfinite(vol).all()
    # SURVEY section 8(d) defines the metric from the H2D copy of the LDCT batch on: the same K steps once more with the batch
    # copied from PINNED host memory inside the timed region (1 MiB per slice).  Reported beside `value`, which keeps the
    # bench contract's definition (inputs resident in HBM when the timed region starts).
    h2d = None
    if a.full and world == 1 and a.sampler == "ddim":
        x_host = x.cpu().pin_memory()
        x_dev = torch.empty_like(x)

        def step_h2d():
            x_dev.copy_(x_host, non_blocking=True)
            return dif.sample([x_dev], batch_size=B, noise=noise, slice_seeds=seeds)[-1]
        step_h2d()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(a.steps):
            vol2 = step_h2d()
        torch.cuda.synchronize()
        dt2 = time.perf_counter() - t1
        h2d = {"value": round(B * a.steps / dt2, 4), "unit": "slices/s", "ms_per_step": round(dt2 / a.steps * 1e3, 2),
               "h2d_bytes_per_step": int(x_host.numel() * x_host.element_size()), "host_memory": "pinned",
               "same_output_as_resident_run": bool(torch.equal(vol2, vol))}

    if rank == 0:
        slices = world * B * a.steps
        res = {
            "metric": f"denoised CT slices/sec (512x512, {a.ddim_steps} DDIM steps)",
            "value": round(slices / dt, 4), "unit": "slices/s", "n_gpus": world, "steps": a.steps,
            "warmup": a.warmup, "ms_per_step": round(dt / a.steps * 1e3, 2), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None,
            "dtype": {"bf16": "bf16", "fp16": "f16 (IEEE binary16 storage and MFMA operands, f32 accumulation)",
                      "fp8": "bf16 activations, e4m3 weights (fp8 MFMA) in the 3x3 convs"}[a.precision]
                     + (f"; last {dif.final_fp32_steps} step(s): "
                        + (f"resolution levels 0-{dif.final_outer_levels - 1}" if dif.final_outer_levels else "whole forward")
                        + (" on the fp32s engine (fp32 storage, split-bf16 contractions: 3 bf16 MFMAs per product)"
                           if a.precision in ("bf16", "fp16") else " in bf16") if dif.final_fp32_steps else ""),
            "data": "synthetic",
            "config": {"workload": "BASELINE configs[2]: 512x512 slice, 50-step DDIM, full FoundDiff UNet "
                                   "(dim 64, mults 1-2-4-8) + DA-CLIP RN50 cond, bf16",
                       "slices_per_gpu_per_step": B, "concurrent_sub_batches": (dif.streams if B >= 8 and B % dif.streams == 0 else 1),
                       "sharding": f"slices over {world} rank(s), no data-path "
                       "collective; 1 all-gather of the output volume"},
            "ms_per_unet_forward_per_slice": round(dt / a.steps / a.ddim_steps / B * 1e3, 3),
            "alg_tflops_sustained": round(ALG_GFLOP_PER_FORWARD * a.ddim_steps * slices / dt / 1e3, 1),
            "inputs": "resident in HBM when the timed region starts (bench contract); `h2d_inclusive` (--full) repeats the region with the "
                      "pinned-host -> device copy of the LDCT batch inside it (SURVEY section 8d)",
            "h2d_inclusive": h2d,
            "box_during_untimed_replay": smi.summary() if smi else None,
            "box_sampler_active_in_timed_region": False,
        }
        if a.sampler == "ancestral":
            res["metric"] = "denoised CT slices/sec (512x512, 1000-step ancestral p_sample_loop)"
            res["config"]["workload"] = ("BASELINE configs[3] sampler: 512x512 slices, 1000-step ancestral p_sample, step noise "
                                         "keyed per slice, full FoundDiff UNet + DA-CLIP RN50 cond, bf16")
        elif a.precision == "fp16" and a.ddim_steps == S_DDIM:
            res["config"]["workload"] = ("BASELINE configs[2] geometry: 512x512 slice, 50-step DDIM, full FoundDiff UNet + DA-CLIP RN50 "
                                         "cond, on the library's IEEE-binary16 build (precision fp16; a variant, not the headline)")
        elif a.precision != "bf16" or a.ddim_steps != S_DDIM:
            res["config"]["workload"] = (f"BASELINE configs[4] geometry: 512x512 slice, {a.ddim_steps}-step DDIM, full FoundDiff "
                                         f"UNet + DA-CLIP RN50 cond, precision {a.precision}")
        if a.full and not a.no_roofline and a.precision == "bf16":
            res["roofline"] = roofline_leg(dif, x, noise, t_measured_ms=res["ms_per_unet_forward_per_slice"],
                                           clock_replay=not a.no_clock_replay)
        if a.full and world == 1 and not a.no_extra_legs and a.precision == "bf16" and a.sampler == "ddim":
            res["fp8_25step"] = fp8_leg(dev, x, noise)
            res["ancestral_config3"] = ancestral_leg(dev, x)
            res["latency_b1"] = latency_leg(dev, x, noise)
        if a.full and world == 1 and not a.no_fp32_leg and a.precision == "bf16":
            # the 16-bit engine on the binary16 build: the bf16 mode's speed class at L2 <= 1e-3 against the oracle over the loop
            res["fp16_mode"] = fp32_parity_leg(dev, x, noise, steps=2, precision="fp16")
            res["fp32s_parity_mode"] = fp32_parity_leg(dev, x, noise, precision="fp32s")
            res["fp32_parity_mode"] = fp32_parity_leg(dev, x, noise)
        if a.full and world == 1 and not a.no_cpu_baseline:
            res["cpu_baseline"] = cpu_baseline_leg(w, x, noise)
        print(json.dumps(res), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
