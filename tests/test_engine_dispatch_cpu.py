"""DAEngine.mamba_block's dispatch against its recorded snapshot (tests/engine_dispatch.py, tests/golden/engine_dispatch.json):
for every configuration and seed, the launches a weight-less engine issues into a recording fake library -- names, every
argument, which pointers alias, probe tags, workspace keys -- are the recorded ones.  Runs on the CPU; touches no kernel."""
import json

import pytest

import engine_dispatch as ED


@pytest.fixture(scope="module")
def gold():
    with open(ED.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def runs():
    """every (configuration, seed), run once: {configuration: [(name sequences, digest, query names) per seed]}"""
    return {cfg: [ED.run(cfg, seed) for seed in ED.SEEDS] for cfg in ED.CONFIGS}


@pytest.mark.parametrize("cfg", list(ED.CONFIGS))
def test_dispatch_matches_snapshot(gold, runs, cfg):
    assert gold["cases"] == ["c%d-%dx%d" % c for c in ED.CASES]
    expect = gold["runs"][cfg]
    assert len(expect) == len(runs[cfg]) == len(ED.SEEDS)                      # no (configuration, seed) skipped
    bad = []
    for seed, (seqs, digest, _) in zip(ED.SEEDS, runs[cfg]):
        want_idx, want_digest = expect[seed]
        for case, s, wi in zip(gold["cases"], seqs, want_idx):
            want = [gold["names"][i] for i in gold["sequences"][wi]]
            if s != want:
                bad.append(f"{cfg} seed {seed} {case}: launched\n    {s}\n  recorded\n    {want}")
        if digest != want_digest and not bad:
            full = [ED.run_block(cfg, seed, *c)[1] for c in ED.CASES]
            bad.append(f"{cfg} seed {seed}: the launch names are the recorded ones; their arguments, aliasing, probes or workspace "
                       f"keys are not (digest {digest}, recorded {want_digest}).  Got\n"
                       + "\n".join(f"  {c}:\n" + "\n".join(f"    {json.dumps(l)}" for l in r["launches"]) + f"\n    bufs {json.dumps(r['bufs'])}"
                                   for c, r in zip(gold["cases"], full)))
        if len(bad) >= 3:
            break
    assert not bad, "\n".join(bad)


def test_snapshot_covers_the_dispatch(gold, runs):
    """every launch and every plan query in mamba_block's source is reached, and the number of distinct launch sequences is
    the recorded one"""
    names, queries, sequences = set(), set(), set()
    for per_seed in runs.values():
        for seqs, _, q in per_seed:
            queries |= q
            for s in seqs:
                names |= set(s)
                sequences.add(tuple(s))
    launches, asked = ED.source_names()
    assert len(launches) >= 15
    assert launches <= names, sorted(launches - names)
    assert asked <= queries, sorted(asked - queries)
    assert sorted(names) == gold["names"]
    assert sorted(queries) == gold["queries"]
    assert len(sequences) == gold["n_sequences"] == len(gold["sequences"])
