"""ResidualDiffusion._sample's routing against its recorded snapshot (tests/sample_routing.py, tests/golden/sample_routing.json):
for every case, the sampler reached, its shapes, which arguments are None, and the draws of x_T and of the seeds in order are the
recorded ones; and _drop_graphs empties every engine's one graph cache.  Runs on the CPU; touches no kernel."""
import json
import types

import pytest

import sample_routing as SR


@pytest.fixture(scope="module")
def gold():
    with open(SR.GOLDEN) as f:
        return json.load(f)


def test_routing_matches_snapshot(gold):
    got = SR.snapshot()
    assert len(SR.CASES) == 512 and list(got) == list(gold)                    # no case skipped
    bad = [f"{k}: routed\n    {json.dumps(got[k])}\n  recorded\n    {json.dumps(gold[k])}" for k in gold if got[k] != gold[k]]
    assert not bad, f"{len(bad)} of {len(gold)} cases differ\n" + "\n".join(bad[:3])


def test_snapshot_distinguishes_the_routes(gold):
    """every sampler is reached, and the two recorded oddities are in the snapshot: the group split of the ancestral sampler
    without seeds draws them twice, and 40 slices on 2 x 16 split into 32 + 8"""
    reached = {r[0] for rows in gold.values() for r in rows}
    assert reached == {"randint", "randn", "_keyed_noise", "ddim_sample", "p_sample_loop", "_sample_concurrent", "returns"}
    rows = gold["S=1000 B=40 streams=2 msb=16 noise=0 seeds=0 step_noise=0 last=1"]
    assert [r[0] for r in rows] == ["randint", "_keyed_noise", "randint", "_sample_concurrent", "_sample_concurrent", "returns"]
    assert [r[1][0] for r in rows[3:5]] == [32, 8]


def test_drop_graphs_empties_every_kind_on_every_engine():
    from founddiff_amd.DADiff import ResidualDiffusion

    def eng():
        return types.SimpleNamespace(graphs={"step": (1, 2), "ddim_loop": (3, 4), "anc": (5, 6)})
    u0 = types.SimpleNamespace(_engine={("bf16", 0): eng(), ("bf16", 1): eng(), ("fp32s", 0): eng()})
    u1 = types.SimpleNamespace(_engine={("bf16", 0): eng()})
    ResidualDiffusion._drop_graphs(types.SimpleNamespace(model=types.SimpleNamespace(unet0=u0, unet1=u1)))
    engines = list(u0._engine.values()) + list(u1._engine.values())
    assert len(engines) == 4 and all(e.graphs == {} for e in engines)
    ResidualDiffusion._drop_graphs(types.SimpleNamespace(model=types.SimpleNamespace(unet0=types.SimpleNamespace(_engine=None))))
