"""Trainer(data_parallel=True) against the single process: tests/_dp_train_worker.py under torch.distributed.run with two ranks
(nccl on two devices where the box has them, otherwise gloo with both ranks on cuda:0) at A = 1, against single-process runs with
gradient_accumulate_every = 2 made here with the worker's own builders.  W ranks x A micro-batches is, bit for bit, the single
process with A W micro-batches: torch.equal on every parameter, EMA tensor and optimiser tensor, equal counters and logged losses,
equal fingerprints on both ranks.  Then a resume from W = 2 into one process, and W = 1 over nccl (the device all-gather route on a
one-GPU box) against the plain path.  The subprocesses take tens of seconds, most of it process start."""
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _launch(out_dir, mode, world):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(HERE, "_dp_train_worker.py"), str(out_dir), mode]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def _worker():
    sys.path.insert(0, HERE)
    import _dp_train_worker as wk
    return wk


def _same(got, want, what):
    """the tensors, the counters and the logged losses of two runs"""
    assert sorted(got["tensors"]) == sorted(want["tensors"]), what
    bad = [k for k in want["tensors"] if not torch.equal(got["tensors"][k], want["tensors"][k])]
    assert not bad, (what, len(bad), bad[:5])
    assert got["counters"] == want["counters"], what
    assert got["losses"] == want["losses"] and len(want["losses"]) == want["counters"][0], (what, got["losses"], want["losses"])


@pytest.fixture(scope="module")
def w2(tmp_path_factory):
    """one worker run with two ranks: the three configurations and the checkpoint of the resume"""
    out = tmp_path_factory.mktemp("dp_w2")
    _launch(out, "w2", 2)
    load = lambda name: [torch.load(out / f"{name}_rank{r}.pt", weights_only=False) for r in range(2)]
    res = {name: load(name) for name in _worker().CONFIGS + ("resume",)}
    res["dir"] = out
    return res


@pytest.fixture(scope="module")
def host_single(tmp_path_factory):
    """the single process on the host configuration, gradient_accumulate_every = 2: its state after 2, 3 and 4 steps"""
    wk = _worker()
    tr = wk.trainer(tmp_path_factory.mktemp("dp_single_host"), 2, "host")
    out = {}
    for steps in (2, 3, 4):
        tr.train_num_steps = steps
        tr.train()
        out[steps] = wk.state(tr)
    return out


def test_two_ranks_really_ran(w2):
    two_devices = torch.cuda.device_count() >= 2
    for name in _worker().CONFIGS:
        ranks = w2[name]
        assert [r["world"] for r in ranks] == [2, 2]
        assert [r["backend"] for r in ranks] == (["nccl"] * 2 if two_devices else ["gloo"] * 2)
        assert [r["device"] for r in ranks] == ([0, 1] if two_devices else [0, 0])
        # a rank drew its own micro-batch of each step: A = 1, so one list per step, and the two ranks' lists differ
        assert all(len(r["batch_log"]) == 3 for r in ranks) and ranks[0]["batch_log"] != ranks[1]["batch_log"]


def test_host_dataset(w2, host_single):
    for r, got in enumerate(w2["host"]):
        _same(got, host_single[3], f"host dataset, rank {r}")
    fp = [got["fingerprints"] for got in w2["host"]]
    assert fp[0] == fp[1] and len(fp[0]) == 2 and fp[0][0] == fp[0][1]
    # the single process drew, micro-batch by micro-batch, what the two ranks drew between them
    single = host_single[3]["batch_log"]
    assert [single[2 * s + r] for s in range(3) for r in range(2)] == \
        [w2["host"][r]["batch_log"][s] for s in range(3) for r in range(2)]


@pytest.mark.parametrize("config", ["store", "two"])
def test_store_and_two_unets(w2, config, tmp_path):
    wk = _worker()
    tr = wk.trainer(tmp_path, 3, config)
    tr.train()
    want = wk.state(tr)
    if config == "two":
        assert len(want["losses"][0][1]) == 2                              # one logged loss per U-Net
    for r, got in enumerate(w2[config]):
        _same(got, want, f"{config}, rank {r}")
    fp = [got["fingerprints"] for got in w2[config]]
    assert fp[0] == fp[1] and fp[0][0] == fp[0][1]
    assert tr.fingerprint() == fp[0][0]                                    # and it is the single process's fingerprint too


def test_resume_in_a_single_process(w2, host_single):
    """2 steps at W = 2, A = 1 and save(); one process with gradient_accumulate_every = 2 loads and runs 2 more: 4 single steps"""
    wk = _worker()
    folder = w2["dir"] / "resume"
    assert os.path.exists(folder / "sample" / "model-1.pt")
    for r, got in enumerate(w2["resume"]):
        _same(got, host_single[2], f"before the save, rank {r}")
    data = torch.load(folder / "sample" / "model-1.pt", map_location="cpu", weights_only=False)
    assert sorted(data) == ["ema", "model", "opt0", "scaler", "step"] and data["step"] == 2      # the keys do not change
    tr = wk.trainer(folder, 4, "host")
    tr.load(1, for_training=True)
    assert tr.step == 2
    tr.train()
    got, want = wk.state(tr), host_single[4]
    bad = [k for k in want["tensors"] if not torch.equal(got["tensors"][k], want["tensors"][k])]
    assert not bad, bad[:5]
    assert got["counters"] == want["counters"] and got["losses"] == want["losses"][2:]


def test_one_rank_over_nccl(tmp_path, host_single):
    """data_parallel=True at W = 1 over nccl: the device all-gather route, against the plain path"""
    _launch(tmp_path, "w1", 1)
    got = torch.load(tmp_path / "w1_rank0.pt", weights_only=False)
    assert got["backend"] == "nccl" and got["world"] == 1 and len(got["fingerprints"]) == 1
    _same(got, host_single[3], "W = 1 over nccl")
    assert got["batch_log"] == host_single[3]["batch_log"]
