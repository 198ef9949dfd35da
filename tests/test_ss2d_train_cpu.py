"""The trainable SS2D mixer's host side, without a GPU: the C ABI of both builds of the library (csrc/fd_ss2d_train.hip and the
NHWC entries of csrc/fd_cross_scan_bwd.hip), founddiff_amd.ss2d_train.SS2D against the reference's captured state dicts, the
argument checks of ss2d_core_fn / ss2d_forward, and the scratch of the new kernels."""
import re
import shutil

import pytest
import torch

NEW_SYMBOLS = ("fd_cross_scan_fwd_nhwc_f32", "fd_cross_scan_bwd_nhwc_f32", "fd_dwconv3x3_silu_bwd_ws_floats",
               "fd_dwconv3x3_silu_bwd_f32", "fd_ln_silu_gate_fwd_f32", "fd_ln_silu_gate_bwd_ws_floats", "fd_ln_silu_gate_bwd_f32")
TAGS = {"c32n4": (32, 4), "c64n32": (64, 32), "c32n16": (32, 16)}


def test_both_libraries_export_the_new_entries():
    from founddiff_amd import _lib as L
    for build in (L.BF16, L.F16):
        lib = build.lib()
        for name in NEW_SYMBOLS:
            assert name in L.SIGNATURES and hasattr(lib, name), name


def test_workspace_sizes_at_level0():
    """down0 of the training shape (batch 2, 512 x 512, d_inner 128, N 4, R 4); nothing for shapes the kernels do not serve"""
    from founddiff_amd import _lib as L
    for build in (L.BF16, L.F16):
        lib = build.lib()
        n = lib.fd_dwconv3x3_silu_bwd_ws_floats(2, 512, 512, 128)
        assert n > 0 and n % 4 == 0
        assert n >= 10 * 128 + 9 * 128              # at least one partial row of dweight | dbias and the mirrored taps
        assert lib.fd_dwconv3x3_silu_bwd_ws_floats(2, 512, 512, 96) == 0
        assert lib.fd_dwconv3x3_silu_bwd_ws_floats(0, 512, 512, 128) == 0
        n = lib.fd_ln_silu_gate_bwd_ws_floats(2, 512 * 512, 128)
        assert n > 0 and n % 4 == 0
        assert n >= 2 * 3 * 128                     # dgamma | dbeta | dlocal per slice
        assert lib.fd_ln_silu_gate_bwd_ws_floats(2, 512 * 512, 96) == 0
        assert lib.fd_ln_silu_gate_bwd_ws_floats(0, 512 * 512, 128) == 0
        # the NHWC scan entries share fd_cross_scan_bwd_ws_floats
        n = lib.fd_cross_scan_bwd_ws_floats(2, 512, 512, 128, 4, 4)
        assert n > 0 and n % 4 == 0
        assert lib.fd_cross_scan_bwd_ws_floats(2, 512, 512, 96, 4, 4) == 0
        assert lib.fd_cross_scan_bwd_ws_floats(2, 512, 512, 128, 6, 4) == 0
        assert lib.fd_cross_scan_bwd_ws_floats(2, 512, 512, 128, 4, 3) == 0
        assert lib.fd_cross_scan_bwd_ws_floats(0, 512, 512, 128, 4, 4) == 0


@pytest.mark.parametrize("tag", sorted(TAGS))
def test_module_has_the_references_state_dict(golden, tag):
    """SS2D(d_model, d_state) has exactly the keys and shapes of the reference's captured SS2D weights (twelve tensors) and
    loads them with strict=True"""
    from founddiff_amd.ss2d_train import SS2D
    prefix = f"ss2d_{tag}."
    sd = {k[len(prefix):]: v for k, v in golden("modules").weights(prefix).items()}
    assert len(sd) == 12
    m = SS2D(*TAGS[tag])
    own = m.state_dict()
    assert set(own) == set(sd), set(own) ^ set(sd)
    for k, v in sd.items():
        assert tuple(own[k].shape) == tuple(v.shape), k
    m.load_state_dict(sd, strict=True)
    for k, v in sd.items():
        assert torch.equal(m.state_dict()[k], v), k


def _core_args(D=64, N=4, R=4, H=8, W=8, B=1):
    return dict(xz=torch.randn(B, H, W, 2 * D), conv_weight=torch.randn(D, 1, 3, 3), conv_bias=torch.randn(D),
                x_proj_weight=torch.randn(4, R + 2 * N, D), dt_projs_weight=torch.randn(4, D, R), dt_projs_bias=torch.randn(4, D),
                A_logs=torch.randn(4 * D, N), Ds=torch.ones(4 * D), norm_weight=torch.ones(D), norm_bias=torch.zeros(D),
                local=torch.randn(B, D))


def test_core_rejects_before_cuda_is_initialised():
    from founddiff_amd import ss2d_train as sst
    was = torch.cuda.is_initialized()
    with pytest.raises(RuntimeError, match="GPU"):
        sst.ss2d_core_fn(**_core_args())
    with pytest.raises(RuntimeError, match="must be a tensor"):
        sst.ss2d_core_fn(**dict(_core_args(), Ds=None))
    # types and shapes are checked before devices
    with pytest.raises(RuntimeError, match="inconsistent shapes"):
        sst.ss2d_core_fn(**dict(_core_args(), conv_weight=torch.randn(64, 1, 5, 5)))
    with pytest.raises(RuntimeError, match="inconsistent shapes"):
        sst.ss2d_core_fn(**dict(_core_args(), x_proj_weight=torch.randn(4, 11, 64)))
    with pytest.raises(RuntimeError, match="inconsistent shapes"):
        sst.ss2d_core_fn(**dict(_core_args(), local=torch.randn(2, 64)))
    with pytest.raises(RuntimeError, match="inconsistent shapes"):
        sst.ss2d_core_fn(**dict(_core_args(), xz=torch.randn(1, 8, 8, 64)))
    with pytest.raises(RuntimeError, match="unsupported shape"):
        sst.ss2d_core_fn(**_core_args(D=96))
    with pytest.raises(RuntimeError, match="unsupported shape"):
        sst.ss2d_core_fn(**_core_args(N=6))
    with pytest.raises(RuntimeError, match="unsupported shape"):
        sst.ss2d_core_fn(**_core_args(R=3))
    with pytest.raises(RuntimeError, match="float32"):
        sst.ss2d_core_fn(**dict(_core_args(), Ds=torch.ones(256, dtype=torch.float64)))
    assert torch.cuda.is_initialized() == was


def test_forward_rejects_unsupported_module_settings():
    """d_conv != 3, ssm_low_rank, a non-LayerNorm out_norm, step_size != 2 and CPU tensors raise RuntimeError before anything
    touches the GPU"""
    from founddiff_amd.ss2d_train import SS2D
    was = torch.cuda.is_initialized()
    x, c = torch.randn(1, 8, 8, 32), torch.randn(1, 1, 256)

    def module(**attrs):
        m = SS2D(32, 4)
        for k, v in attrs.items():
            setattr(m, k, v)
        return m
    with pytest.raises(RuntimeError, match="GPU"):
        module()(x, c)
    with pytest.raises(RuntimeError, match="d_conv"):
        module(d_conv=5)(x, c)
    with pytest.raises(RuntimeError, match="ssm_low_rank"):
        module(ssm_low_rank=True)(x, c)
    with pytest.raises(RuntimeError, match="step_size"):
        module(step_size=1)(x, c)
    with pytest.raises(RuntimeError, match="out_norm"):
        module(out_norm=torch.nn.Sigmoid())(x, c)
    with pytest.raises(RuntimeError, match="out_norm"):
        module(out_norm=torch.nn.LayerNorm(64, elementwise_affine=False))(x, c)
    with pytest.raises(RuntimeError, match="depthwise 3x3"):
        module(conv2d=torch.nn.Conv2d(64, 64, 5, padding=2, groups=64))(x, c)
    assert torch.cuda.is_initialized() == was


def test_new_kernels_use_no_scratch():
    """0 bytes of scratch per lane for every kernel of csrc/fd_ss2d_train.hip, and for the cross-scan kernels that gained the NHWC
    dx path, in both builds (hipcc's kernel-resource-usage remarks, founddiff_amd.build.resources())"""
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    from founddiff_amd import build
    for half in ("bf16", "fp16"):
        build.build(half=half)
        res = build.resources(half)
        tab = res.get("fd_ss2d_train.hip")
        assert tab, "no resource remarks beside fd_ss2d_train.hip's object: rebuild with build(force=True)"
        seen = set()
        for name, r in tab.items():
            assert r.get("scratch", 0) == 0, (half, name, r)
            m = re.search(r"(partial_sum_kernel|dwb_pre_kernel|dwb_flip_kernel|lsg_fwd_kernel|lsg_bwd_kernel|lsg_finish_kernel)", name)
            if m:
                seen.add(m.group(1))
        assert seen == {"partial_sum_kernel", "dwb_pre_kernel", "dwb_flip_kernel", "lsg_fwd_kernel", "lsg_bwd_kernel",
                        "lsg_finish_kernel"}, seen
        cs = {n: r for n, r in res["fd_cross_scan_bwd.hip"].items() if re.search(r"cs_scan_kernel|cs_xproj_kernel", n)}
        assert len(cs) == 100                       # 20 (N, R) pairs x (carry, main and x_proj in both dx layouts)
        for name, r in cs.items():
            assert r.get("scratch", 0) == 0, (half, name, r)
