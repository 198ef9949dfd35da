"""The samplers' launch order against its recorded snapshot (tests/sample_launches.py, tests/golden/sample_launches.json): for every
case the kernels and engine methods reached, in order, with their scalar arguments and the names of the buffers behind their
pointers, the graphs captured and replayed, what was raised or warned and the state left behind.  Runs on the CPU; touches no kernel."""
import json

import pytest

import sample_launches as SL


@pytest.fixture(scope="module")
def gold():
    with open(SL.GOLDEN) as f:
        return json.load(f)


def _flat(rows):
    """the folded rows, unfolded"""
    out = []
    for r in rows:
        out.extend(_flat(r[2]) * r[1] if r[0] == "x" else [r])
    return out


def _first_difference(a, b):
    a, b = _flat(a), _flat(b)
    i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return f"row {i} of {len(a)} / {len(b)}: launched\n    {json.dumps(a[i:i + 1])}\n  recorded\n    {json.dumps(b[i:i + 1])}"


def test_launches_match_snapshot(gold):
    got = SL.snapshot()
    assert list(got) == list(gold) == list(SL.CASES)                           # no case skipped
    bad = [f"{k}: {_first_difference(got[k], gold[k])}" for k in gold if got[k] != gold[k]]
    assert not bad, f"{len(bad)} of {len(gold)} cases differ\n" + "\n".join(bad[:5])


def _names(rows):
    return {r[0] for r in _flat(rows)}


def _kinds(rows):
    return {r[2] for r in _flat(rows) if r[0] == "captured"}


def _state(rows):
    return next(r for r in rows if r[0] == "state")


def test_snapshot_covers_every_path(gold):
    """every loop, entry point and chunk shape the snapshot is there for is in it"""
    kinds = {k: _kinds(v) for k, v in gold.items()}
    assert set().union(*kinds.values()) == {"step", "ddim_loop", "anc", "obj_ddim", "obj_anc"}
    names = set().union(*(_names(v) for v in gold.values()))
    assert names >= {"fd_res_ddim_step", "fd_ancestral_begin", "fd_res_posterior_step_keyed", "fd_res_posterior_step", "fd_obj_begin",
                     "fd_res_step_obj_keyed", "fd_res_step_obj", "fd_rows_repeat_f32", "fd_tiles_blend_f32", "fd_tiles_gather_f32",
                     "fd_tiles_step_ddim_f32", "fd_tiles_step_keyed_f32", "fd_keyed_normal", "fd_axpy_f32", "ensemble_stats",
                     "forward", "forward_hybrid", "encode_condition", "encode_dose", "condition_from", "load_condition",
                     "share_condition", "time_table_prepare", "time_cond_table", "replay", "raises", "warns"}
    # shipped DDIM captured and eager; shipped ancestral keyed and with step_noise, last true and false
    assert kinds["ddim captured hybrid-tail"] == {"ddim_loop"} and kinds["ddim eager step-graphs trajectory"] == {"step"}
    assert not kinds["ddim eager no-graph"] and "fd_res_ddim_step" in _names(gold["ddim eager no-graph"])
    assert kinds["anc keyed T=84"] == {"anc"} and not kinds["anc keyed T=6 trajectory"]
    for k in ("anc step_noise T=5", "anc step_noise T=5 trajectory"):
        assert kinds[k] == {"step"} and "fd_res_posterior_step" in _names(gold[k])
    # the chunk shapes of the ancestral loops: rem > 0 with reps > 1 and no divisor (G = 40), a divisor, reps = 0, a tail, the limit
    replays = lambda k: [r for r in _flat(gold[k]) if r[0] == "replay"]
    count = lambda k, name: sum(1 for r in _flat(gold[k]) if r[0] == name)
    assert len(replays("anc keyed T=84")) == 3 and _state(gold["anc keyed T=84"])[1] == 84
    assert len(replays("anc keyed T=84 max-chunks")) == 2 and _state(gold["anc keyed T=84 max-chunks"])[1] == 41
    assert _state(gold["anc keyed T=84 max-chunks"])[2] == {"unet0/bf16/0:loop_t": 1}                # the jump to the tail
    assert len(replays("anc keyed T=17 noise")) == 2 and len(replays("anc keyed T=6")) == 1
    assert len(replays("obj_anc res_noise T=83")) == 2 and _state(gold["obj_anc res_noise T=83"])[1] == 83
    assert len(replays("obj_anc res_noise T=83 max-chunks")) == 1 and _state(gold["obj_anc res_noise T=83 max-chunks"])[1] == 40
    assert _state(gold["obj_anc pred_noise T=83 no-graph max-chunks"])[1] == 40
    assert count("anc keyed T=84", "fd_ancestral_begin") == 3 + 40 + 1         # rem eager steps, the chunk's graph, the tail's
    # every plan on both captured loops and on the eager one
    for plan in ("pred_noise", "res_noise", "rn_noise"):
        assert kinds[f"obj_ddim {plan}"] == {"obj_ddim"} and kinds[f"obj_anc {plan} T=83"] == {"obj_anc"}
        assert not kinds[f"generic ddim {plan} trajectory"] and not kinds[f"generic anc {plan} trajectory"]
        assert "fd_res_step_obj" in _names(gold[f"generic ddim {plan} trajectory"]) & _names(gold[f"generic anc {plan} trajectory"])
    # (two U-Nets with test_res_or_noise='res' are the shipped plan: unet0 alone, on the shipped loops)
    assert kinds["obj_ddim rn_res"] == {"ddim_loop"} and kinds["obj_anc rn_res T=83"] == {"anc"}
    # ensembles and tiles, both fuse modes, both values of condition, both samplers
    assert sum(1 for r in _flat(gold["ensemble ddim msb=1"]) if r[0] == "encode_condition") == 2
    for fuse in ("final", "step"):
        for cond in ("tile", "slice"):
            for smp in ("ddim", "anc"):
                assert ("encode_dose" in _names(gold[f"tiled {fuse} {cond} {smp}"])) == (cond == "slice")
                assert ("fd_tiles_blend_f32" in _names(gold[f"tiled {fuse} {cond} {smp}"])) == (fuse == "final")
    # tiled ensembles: the tower never runs per replica; "final" reduces the tile rows in one launch, whose samples pointer is
    # null unless the images are asked for (quantiles ask); "step" goes through ensemble_stats; the order kernel sees K images
    for fuse in ("final", "step"):
        for cond in ("tile", "slice"):
            for smp in ("ddim", "anc", "ddim res_noise", "anc res_noise"):
                rows = gold[f"ensemble tiled {fuse} {cond} {smp}"]
                assert ("encode_dose" in _names(rows)) == (cond == "slice")
                assert ("fd_tiles_ensemble_f32" in _names(rows)) == (fuse == "final") == ("ensemble_stats" not in _names(rows))
                assert ("fd_tiles_step_ddim_f32" in _names(rows) or "fd_tiles_step_keyed_f32" in _names(rows)) == (fuse == "step")
                assert "fd_tiles_blend_f32" not in _names(rows)
    reduce_of = lambda k: next(r for r in _flat(gold[k]) if r[0] == "fd_tiles_ensemble_f32")
    assert reduce_of("ensemble tiled final tile ddim no-samples")[6] is None
    assert reduce_of("ensemble tiled final tile ddim")[6] is not None and reduce_of("ensemble quantiles tiled final")[6] is not None
    assert ["returns", [[2, 1, 8, 8], [2, 1, 8, 8], [2], None]] in gold["ensemble tiled final tile ddim no-samples"]
    for k in ("ensemble quantiles ddim msb=4", "ensemble quantiles tiled final", "ensemble quantiles tiled step"):
        assert ["ensemble_quantiles", [2, 3, 1, 8, 8], [0.05, 0.5, 0.95]] in gold[k]
    assert _state(gold["ensemble tiled step tile anc pred_noise T=83 max-chunks"])[1] == 40
    # the range check of the entry points: 'fp16' raises, 'auto' warns, sets _auto_bf16 and runs again on the bf16 engines
    for what in ("sample", "ensemble", "tiled final", "tiled step", "ensemble tiled final", "ensemble tiled step"):
        rows = gold[f"fallback {what} fp16"]
        assert "raises" in _names(rows) and ["returns", None] in rows and ["_auto_bf16", [False]] in rows
        rows = _flat(gold[f"fallback {what} auto"])
        assert "warns" in _names(rows) and "raises" not in _names(rows) and ["_auto_bf16", [True]] in rows
        engines = [r[1] for r in rows if r[0] == "forward"]
        assert engines[0] == "unet0/fp16/0" and engines[-1].startswith("unet0/") and "unet0/bf16/0" in engines
