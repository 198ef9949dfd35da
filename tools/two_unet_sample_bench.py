"""Sampling the two-U-Net and pred_noise models (ResidualDiffusion._obj_ddim / _obj_ancestral, csrc/fd_sched.hip): what the captured
loops, the device-side step bookkeeping and the two streams buy over the eager single-stream form of the same launches.  Everything
is reported, nothing is gated.  The shipped architecture Unet(64, (1, 2, 4, 8)) with synthetic weights, 512 x 512, bf16.

  ddim_b1 / ddim_b8 / ddim_b32   two U-Nets under 'pred_res_noise' / 'res_noise', 50 DDIM steps, 1, 8 and 32 slices
  anc_b8                         the same model, the ancestral sampler bounded to one chunk of 50 steps (_anc_max_chunks), 8 slices
  pred_noise_b8                  one U-Net under 'pred_noise', 50 DDIM steps, 8 slices
  step_kernel                    fd_res_step_obj_keyed alone (mode 2, 8 slices): milliseconds from device events around --inner
                                 back-to-back calls, the bytes it moves (three streams read, one written) and those over 6.3 TB/s

Every sampling leg times `new` = sample() as it is (use_graph=True, the model's streams) against `old` = the same call on a second
model of the same weights with use_graph=False and streams=1: the same launches issued eagerly on one stream, which is what these
models ran before the captured loops, up to a clone per model output.  Wall milliseconds per call to the closing synchronisation,
the two alternated inside one loop, --reps timed rounds after two untimed ones (the first packs the engines and captures the loops,
the second counts the C-ABI calls the host makes, L.TRACE), the median reported with every sample.  x_T and the seeds are given, so
the two images can be compared bit for bit.  Two models, because an engine keeps one loop graph per kind and the two forms put
different batch sizes on it.  Each leg runs in a child process of its own under its own time limit; the first leg that fails or
runs out of time ends the tool.

    python tools/two_unet_sample_bench.py [--reps 3] [--inner 20] [--steps 50] [--legs ddim_b1,...] [--limit 420] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BPS = 6.3e12
LEGS = ("ddim_b1", "ddim_b8", "ddim_b32", "anc_b8", "pred_noise_b8", "step_kernel")
SIZE = 512


def _model(two, steps, dev):
    import torch  # noqa: F401
    from founddiff_amd import arch, synth
    from founddiff_amd.DADiff import ResidualDiffusion, UnetRes, load_weights
    nu, obj, tst = (2, "pred_res_noise", "res_noise") if two else (1, "pred_noise", "noise")
    w = {}
    for i in range(nu):
        w.update(synth.synth_state_dict(arch.da_unet_spec(64, (1, 2, 4, 8), prefix=f"model.unet{i}."), seed=i))
    net = UnetRes(dim=64, dim_mults=(1, 2, 4, 8), num_unet=nu, condition=True, objective=obj, test_res_or_noise=tst, precision="bf16")
    dif = ResidualDiffusion(net, image_size=SIZE, timesteps=1000, sampling_timesteps=steps, objective=obj, loss_type="l2",
                            condition=True, sum_scale=0.01, test_res_or_noise=tst)
    load_weights(dif, w, "synthetic weights")
    dif = dif.to(dev)
    dif.init()
    return dif


def _workspace_mb(dif):
    engines = [e for u in (getattr(dif.model, "unet0", None), getattr(dif.model, "unet1", None)) if u is not None
               for e in (u._engine or {}).values()]
    return round(sum(e.workspace_bytes() for e in engines) / 1e6, 0), len(engines)


def sampling_leg(name, a):
    import torch
    from founddiff_amd import _lib as L
    from founddiff_amd import synth
    dev = torch.device("cuda:0")
    kind, B = name.rsplit("_b", 1)
    B = int(B)
    anc = kind == "anc"
    steps = 1000 if anc else a.steps
    new, old = _model(kind != "pred_noise", steps, dev), _model(kind != "pred_noise", steps, dev)
    old.use_graph, old.streams = False, 1
    if anc:
        new._anc_max_chunks = old._anc_max_chunks = 1
    x = torch.from_numpy(synth.ct_phantom(B, SIZE, seed=10)[1]).to(dev)
    seeds = torch.arange(B, dtype=torch.int64) + 1000
    nz = new._keyed_noise(seeds.to(dev), new.X_T_STEP, tuple(x.shape))
    out, ms, calls = {}, {"new": [], "old": []}, {}
    for it in range(2 + a.reps):
        for tag, dif in (("new", new), ("old", old)):
            if it == 1:
                L.TRACE = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[tag] = dif.sample([x], batch_size=B, noise=nz, slice_seeds=seeds)[-1]
            torch.cuda.synchronize()
            if it >= 2:
                ms[tag].append((time.perf_counter() - t0) * 1e3)
            if it == 1:
                calls[tag], L.TRACE = len(L.TRACE), None
    med = lambda v: sorted(v)[len(v) // 2]
    nsteps = new._anc_steps_run if anc else steps
    nm, om = med(ms["new"]), med(ms["old"])
    ws_new, n_new = _workspace_mb(new)
    ws_old, n_old = _workspace_mb(old)
    return dict(leg=name, model="two U-Nets pred_res_noise/res_noise" if kind != "pred_noise" else "one U-Net pred_noise",
                sampler="ancestral (bounded)" if anc else "ddim", slices=B, steps=nsteps, size=SIZE, precision="bf16",
                streams_new=new.streams, new_ms=round(nm, 2), old_ms=round(om, 2), new_ms_all=[round(v, 2) for v in ms["new"]],
                old_ms_all=[round(v, 2) for v in ms["old"]], old_over_new=round(om / nm, 3),
                new_slices_per_s=round(B / nm * 1e3, 2), old_slices_per_s=round(B / om * 1e3, 2),
                host_calls_per_step_new=round(calls["new"] / nsteps, 2), host_calls_per_step_old=round(calls["old"] / nsteps, 2),
                workspace_MB_new=ws_new, engines_new=n_new, workspace_MB_old=ws_old, engines_old=n_old,
                process_peak_MB=round(torch.cuda.max_memory_allocated(dev) / 1e6, 0),
                images_bitwise_equal=bool(torch.equal(out["new"], out["old"])),
                max_abs_diff=float((out["new"] - out["old"]).abs().max()), finite=bool(torch.isfinite(out["new"]).all()))


def kernel_leg(a):
    import torch
    from founddiff_amd import _lib as L
    from founddiff_amd.DADiff import residual_schedule
    dev = torch.device("cuda:0")
    B, npix, T, mode = 8, SIZE * SIZE, 1000, 2
    s = residual_schedule(T, after_init=True)
    cols = [s[k] for k in ("alphas_cumsum", "betas_cumsum", "one_minus_alphas_cumsum", "posterior_mean_coef1", "posterior_mean_coef2",
                           "posterior_mean_coef3", "posterior_log_variance_clipped")]
    tab = torch.stack(cols + [torch.zeros(T)], 1).contiguous().to(dev)
    g = torch.Generator().manual_seed(0)
    o0, o1, xt = [torch.randn(B, npix, generator=g).to(dev) for _ in range(3)]
    out = torch.empty(B, npix, device=dev)
    seeds = (torch.arange(B, dtype=torch.int64) + 1000).to(dev)
    t_dev = torch.tensor([500], dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    fn = lambda: L.call("fd_res_step_obj_keyed", mode, o0.data_ptr(), o1.data_ptr(), xt.data_ptr(), None, tab.data_ptr(),
                        t_dev.data_ptr(), seeds.data_ptr(), out.data_ptr(), B, npix, T, st)
    ts = []
    for it in range(2 + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            fn()
        e1.record()
        e1.synchronize()
        if it >= 2:
            ts.append(e0.elapsed_time(e1) / a.inner)
    med = sorted(ts)[len(ts) // 2]
    nbytes = 4 * B * npix * 4                                      # mode 2: o0, o1, x_t read, img_out written
    bound = nbytes / HBM_BPS * 1e3
    return dict(leg="step_kernel", kernel="fd_res_step_obj_keyed", mode=mode, slices=B, size=SIZE, t=500, ms=round(med, 4),
                min_ms=round(min(ts), 4), ms_all=[round(v, 4) for v in ts], MB=round(nbytes / 1e6, 2),
                GBps=round(nbytes / med / 1e6, 0), bound_ms_at_6p3TBps=round(bound, 4), bound_over_ms=round(bound / med, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--limit", type=int, default=420, help="seconds a leg (one child process) may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_unet_sample_bench.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("tools/two_unet_sample_bench.py measures on the GPU: none is visible")
        row = kernel_leg(a) if a.child == "step_kernel" else sampling_leg(a.child, a)
        print("ROW " + json.dumps(row), flush=True)
        return
    legs = [v for v in a.legs.split(",") if v]
    bad = [v for v in legs if v not in LEGS]
    if bad:
        raise SystemExit(f"unknown leg(s) {bad}: choose from {LEGS}")
    rows = []
    for leg in legs:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", leg, "--reps", str(a.reps), "--inner", str(a.inner),
               "--steps", str(a.steps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            rows.append(dict(leg=leg, error=f"no result within {a.limit} s"))
            break
        got = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("ROW ")]
        if r.returncode != 0 or not got:
            rows.append(dict(leg=leg, error=f"exit status {r.returncode}", stderr=r.stderr[-1500:]))
            break                                                  # nothing more is started on the GPU behind a failed leg
        rows.append(json.loads(got[-1]))
        print(f"# {got[-1]}", file=sys.stderr, flush=True)
    res = dict(tool="tools/two_unet_sample_bench.py", reps=a.reps, inner=a.inner, ddim_steps=a.steps, rows=rows)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if any("error" in r for r in rows):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
