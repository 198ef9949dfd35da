"""Characterization of DAEngine.mamba_block's host-side dispatch, on the CPU: a weight-less engine whose library is a
recording fake runs the block under seeded, order-independent answers to every plan query, and what it launched -- names,
arguments, the alias structure of the pointers, probe tags, workspace keys -- is compared with tests/golden/engine_dispatch.json
(tests/test_engine_dispatch_cpu.py).  The golden pins behaviour, not correctness: it was recorded from the engine before
mamba_block was split into named decisions, and a change that is meant to alter the dispatch regenerates it with

    python tests/engine_dispatch.py --write
"""
import ctypes as C
import hashlib
import inspect
import json
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from founddiff_amd import _lib as L, arch, synth                      # noqa: E402
from founddiff_amd.engine import DAEngine, _Sub, _T                   # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "engine_dispatch.json")
SEEDS = range(128)
B = 2
CASES = [(64, 8, 8), (64, 9, 7), (128, 8, 8), (128, 9, 7)]             # (C, H, W): both widths, an even and an odd image
# name -> (mode, the engine flags the stub sets).  No flags = what an engine stub that skips __init__ gets.
CONFIGS = {
    "bf16-defaults": ("bf16", {}),
    "fp32-defaults": ("fp32", {}),
    "bf16-zre-vre": ("bf16", dict(z_recompute=1, v_recompute=True)),
    "bf16-zre-vre-lowlat": ("bf16", dict(z_recompute=1, v_recompute=True, low_latency=True)),
    "bf16-zre64": ("bf16", dict(z_recompute=64, v_recompute=True)),
    "fp32s-z0": ("fp32s", dict(f32_split=1, z_recompute=0)),
    "fp32s-zre": ("fp32s", dict(f32_split=1, z_recompute=1)),
    "fp16-zre-vre": ("fp16", dict(z_recompute=1, v_recompute=True)),
}
_SIZES = {"fd_conv_mtiles": 2, "fd_scan_ws_floats": 40, "fd_pw_dw3x3_gram_f32_nblk": 3, "fd_pw_dw3x3_gram_nblk": 7,
          "fd_pw_dw3x3_gram_nblk_opts": 4, "fd_dwconv_gram_nblk": 5, "fd_chan_attn_nblk": 6}
_PTR_FIELDS = [n for n, t in L.ConvParams._fields_ if t is L.vp]
_VAL_FIELDS = [n for n, t in L.ConvParams._fields_ if t is not L.vp]


class FakeLibrary:
    """Stands where a founddiff_amd._lib.Library does (DAEngine.hip).  lib() answers the plan queries: a boolean one with a hash
    bit of (seed, query name, scalar arguments) -- for the conv probe, every non-pointer field of ConvParams and which pointer
    fields are set -- so the answer does not depend on the order the questions arrive in; a size query with a fixed small
    integer.  call() records the launch."""

    def __init__(self, seed):
        self.seed, self.record, self.queries, self._ptrs = seed, [], set(), {}

    def lib(self):
        return self

    def __getattr__(self, name):
        if not name.startswith("fd_"):
            raise AttributeError(name)

        def query(*args):
            self.queries.add(name)
            if name in _SIZES:
                return _SIZES[name]
            if not (name.endswith("_ok") or name == "fd_selective_scan_plan"):
                raise AssertionError(f"the fake library has no answer for {name}")
            if name == "fd_conv_prologue_ok":
                p = args[0]._obj
                args = [getattr(p, f) for f in _VAL_FIELDS] + [bool(getattr(p, f)) for f in _PTR_FIELDS]
            key = repr((self.seed, name, [a if isinstance(a, bool) else float(a) for a in args]))
            return hashlib.sha256(key.encode()).digest()[0] & 1
        return query

    def _ptr(self, v):
        """address -> index of its first appearance in this run (null stays null)"""
        return None if not v else self._ptrs.setdefault(v, len(self._ptrs))

    def _arg(self, a):
        if a is None:
            return None
        if isinstance(a, C.c_void_p):
            return {"p": self._ptr(a.value)} if a.value else None
        if isinstance(a, (int, float)):
            return a
        p = a._obj                                      # byref(ConvParams): the fields that are set (a zeroed one is its default)
        return {f: ({"p": self._ptr(getattr(p, f))} if f in _PTR_FIELDS else getattr(p, f)) for f, _ in p._fields_ if getattr(p, f)}

    def call(self, name, *args):
        self.record.append([name] + [self._arg(a) for a in args])


def _stub(mode, flags, hip):
    class Stub(DAEngine):
        stream = property(lambda self: None)

        def __init__(self):
            self.mode = mode
            self.dt, self.tdt = _T[mode]
            self.dev = torch.device("cpu")
            self.f32 = dict(device=self.dev, dtype=torch.float32)
            self.buf = {}
            self.hip = hip
            for k, v in flags.items():
                setattr(self, k, v)
            if flags and not isinstance(inspect.getattr_static(DAEngine, "scan_dt", None), property):
                # (an engine from before scan_dt became a property derived from these flags: what its __init__ stored)
                self.scan_dt = (self.dt | (L.FD_OPT_LOW_LATENCY if flags.get("low_latency") else 0)
                                | (L.FD_OPT_F32_SPLIT if flags.get("f32_split") else 0))
    return Stub()


_packed = {}


def _weights(cfg, Cc):
    """the packed Mamba_block of width Cc for a configuration (packing depends on the mode and on f32_split only)"""
    mode, flags = CONFIGS[cfg]
    key = (mode, flags.get("f32_split", 0), Cc)
    if key not in _packed:
        spec = {}
        arch._mamba(spec, "b.", Cc, 4, 256)
        m = _stub(mode, flags, None)._pack_mamba(_Sub(synth.synth_state_dict(spec, seed=3), "b."))
        m["mod_off"], m["loc_off"] = 6, 10
        _packed[key] = m
    return _packed[key]


def run_block(cfg, seed, Cc, H, W):
    """One mamba_block call -> (launch names, the full normalised record, the query names asked)."""
    mode, flags = CONFIGS[cfg]
    fake = FakeLibrary(seed)
    e = _stub(mode, flags, fake)
    m = _weights(cfg, Cc)
    e.mod_total, e.loc_total = 6 * Cc + 14, m["D"] + 18
    e.mod_all = torch.zeros(B, e.mod_total)
    e.local_all = torch.zeros(B, e.loc_total)
    e.probe = lambda tag, t: fake.record.append(["probe", tag, list(t.shape)])
    x = torch.zeros(B, H, W, Cc, dtype=e.tdt)
    out = e.mamba_block(m, x, B, H, W, "blk")
    bufs = sorted([name, list(shape), str(dt)] for name, shape, dt in e.buf)
    full = dict(launches=fake.record, bufs=bufs, out=fake._arg(C.c_void_p(out.data_ptr())), shape=list(out.shape))
    return [r[0] for r in fake.record if r[0] != "probe"], full, fake.queries


def run(cfg, seed):
    """All CASES of one (configuration, seed) -> (the name sequence of each, a digest of the full records, query names)."""
    seqs, fulls, queries = [], [], set()
    for case in CASES:
        names, full, q = run_block(cfg, seed, *case)
        seqs.append(names)
        fulls.append(full)
        queries |= q
    digest = hashlib.sha256(json.dumps(fulls, sort_keys=True).encode()).hexdigest()[:12]
    return seqs, digest, queries


def dispatch_source():
    """source text of mamba_block and of the DAEngine methods it is made of (not the op wrappers every stage shares)"""
    seen, todo = {}, ["mamba_block"]
    while todo:
        n = todo.pop()
        fn = inspect.getattr_static(DAEngine, n, None)
        if n in seen or n in ("_b", "_pr", "conv", "conv_cols", "linear") or not inspect.isfunction(fn):
            continue
        seen[n] = inspect.getsource(fn)
        todo += re.findall(r"self\.(\w+)\(", seen[n])
    return "\n".join(seen.values())


def source_names():
    """(launch names, query names) that appear in the dispatch's source"""
    src = dispatch_source()
    launches = set(re.findall(r'\.call\(\s*"(fd_\w+)"', src)) | ({"fd_conv2d"} if "self.conv(" in src else set())
    queries = set(re.findall(r"\.(fd_\w+)\(", src)) | ({"fd_conv_prologue_ok"} if "probe=True" in src else set())
    return launches, queries


def snapshot():
    names, queries, seqs, runs = set(), set(), {}, {}
    for cfg in CONFIGS:
        runs[cfg] = []
        for seed in SEEDS:
            ss, digest, q = run(cfg, seed)
            queries |= q
            for s in ss:
                names |= set(s)
            runs[cfg].append([[seqs.setdefault(tuple(s), len(seqs)) for s in ss], digest])
    order = sorted(names)
    return dict(cases=["c%d-%dx%d" % c for c in CASES], names=order, queries=sorted(queries), n_sequences=len(seqs),
                sequences=[[order.index(n) for n in s] for s in seqs], runs=runs)


def write(path=GOLDEN):
    g = snapshot()
    with open(path, "w") as f:
        f.write("{\n")
        for k in ("cases", "names", "queries", "n_sequences"):
            f.write(f' "{k}": {json.dumps(g[k])},\n')
        f.write(' "sequences": [\n' + ",\n".join("  " + json.dumps(s, separators=(",", ":")) for s in g["sequences"]) + "\n ],\n")
        f.write(' "runs": {\n' + ",\n".join(f'  "{c}": ' + json.dumps(r, separators=(",", ":")) for c, r in g["runs"].items()))
        f.write("\n }\n}\n")
    return g


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/engine_dispatch.py --write")
    g = write()
    print(f"{GOLDEN}: {len(g['names'])} launch names, {len(g['queries'])} queries, {g['n_sequences']} sequences, "
          f"{os.path.getsize(GOLDEN)} bytes")
