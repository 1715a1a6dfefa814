"""No GPU: the shapes of tests/passbshapes.py plan the chunk counts they are
named for, and ADL_BLOOM_CHUNK_KEYS does what it says.

make_plan (adlsm-tree_amd/csrc/bloom_build.hip) runs on the host and assumes
256 compute units when there is no device, so adl_bloom_build_workspace_bytes
under ADL_BLOOM_DEBUG=1 prints here the plan line a build on an MI355X prints.
Every shape is checked for C, the chunks in all, the tile size, claim or dense
and pass B's workgroups per CU, and from C for each filter's chunk count
ceil(n_f / C): the number of segment batches pass B walks for that filter's
tiles.  tests/test_gpu_pass_b_batches.py asserts the same line on the GPU.
"""
import re

import pytest

from passbshapes import S, S2, SHAPES

PLAN = re.compile(r"adl_bloom plan: filters (\d+), tile 2\^(\d+) bits, tiles (\d+), C (\d+), chunks (\d+), "
                  r"region (\d+) words( \(claim\))?, pass B (\d) per CU")


@pytest.fixture
def planner(knobs, capfd):
    import adlbloom

    def plan(sizes, bpk, env):
        for k, v in env.items():
            knobs.set(k, v)
        knobs.set("ADL_BLOOM_DEBUG", "1")
        capfd.readouterr()
        ws = adlbloom.workspace_bytes(sizes, bpk)
        lines = PLAN.findall(capfd.readouterr().err)
        for k in env:
            knobs.unset(k)
        assert ws > 0 and len(lines) == 1
        nf, tl, tiles, c, chunks, region, claim, occ = lines[0]
        return {"filters": int(nf), "tl": int(tl), "tiles": int(tiles), "C": int(c), "chunks": int(chunks),
                "region": int(region), "claim": bool(claim), "occ": int(occ), "ws": ws}

    return plan


@pytest.mark.parametrize("name", list(SHAPES))
def test_shape_plans_its_chunk_counts(planner, name):
    sh = SHAPES[name]
    p = planner(sh.sizes, sh.bpk, sh.env)
    assert (p["filters"], p["C"], p["tl"], p["claim"], p["occ"]) == (len(sh.sizes), sh.C, sh.tl, sh.claim, sh.occ)
    assert [-(-n // p["C"]) for n in sh.sizes] == sh.chunks
    assert p["chunks"] == sum(sh.chunks)


def test_every_seam_is_in_a_shape():
    """The counts the sweep promises, by pass-B kernel and descriptor source."""
    def counts(names):
        return {w for n in names for w in SHAPES[n].chunks}

    sweep = {1, 15, 16, 17, 255, 256, 257, S - 1, S, S + 1, S + 15, S + 16, S + 17, 2 * S - 1, 2 * S, 2 * S + 1,
             2 * S + 17, 3 * S + 1}
    assert sweep <= counts(["K1", "K2", "K3", "K4"]) and sweep <= counts(["D1", "D2"])
    assert all(len(SHAPES[n].sizes) <= 8 for n in ("K1", "K2", "K3", "K4", "M8"))
    assert all(len(SHAPES[n].sizes) > 8 for n in ("D1", "D2", "M16"))
    assert {S - 1, S, S + 1, 2 * S + 1} <= counts(["C1"]) and SHAPES["C1-tight"].chunks == SHAPES["C1"].chunks
    for n in ("var", "bpk44", "stride24"):
        assert {S + 1, 2 * S + 1} <= counts([n])
    two = {S2 - 1, S2, S2 + 1, S2 + 16, 2 * S2 + 1, 3 * S2 + 1}
    assert two <= counts(["M8", "M16"]) and {S2 - 1, S2, S2 + 1, S2 + 16, 2 * S2 + 1} <= counts(["M8"])
    # an empty and a 1-key filter directly after and directly before a filter of more than one batch
    for n, segb in (("K1", S), ("K2", S), ("D1", S), ("D2", S), ("C1", S), ("M8", S2), ("M16", S2)):
        sz, ch = SHAPES[n].sizes, SHAPES[n].chunks
        assert any(sorted(sz[i:i + 2]) == [0, 1] and ch[i - 1] > segb and ch[i + 2] > segb
                   for i in range(1, len(sz) - 2)), n
    for a, b in (("K1", "K2"), ("M8", "M16")):  # ... in both orders
        assert SHAPES[a].sizes[1:3] == [0, 1] and SHAPES[b].sizes[1:3] == [1, 0]
    # the pass-B grids of the queued two-per-CU cases are multiples of 8 (one tile per bpk-0 filter)
    assert len(SHAPES["M8"].sizes) == 8 and len(SHAPES["M16"].sizes) == 16


BENCH = [  # the benchmark's configs (BASELINE.json): the plan lines before the knob existed
    ([100_000], {"tl": 13, "tiles": 977, "C": 392, "chunks": 256, "region": 2352, "claim": False, "occ": 1,
                 "ws": 4280064}),
    ([10_000_000], {"tl": 20, "tiles": 763, "C": 5584, "chunks": 1791, "region": 33504, "claim": False, "occ": 1,
                    "ws": 325571328}),
    ([1_000_000] * 256, {"tl": 18, "tiles": 78336, "C": 5652, "chunks": 45312, "region": 33912, "claim": False,
                         "occ": 2, "ws": 8253536256}),
]


@pytest.mark.parametrize("sizes,want", BENCH, ids=["100k", "headline", "256x1M"])
def test_knob_not_set_leaves_the_benchmark_plans(planner, sizes, want):
    """configs[0], [1] and [2] (10 M keys: the plan reads counts, not key
    bytes) and [3] and [4] (256 x 1 M).  0 and a value above the plan's own
    bound mean the same as not set."""
    for env in ({}, {"ADL_BLOOM_CHUNK_KEYS": "0"}, {"ADL_BLOOM_CHUNK_KEYS": "1000000000"}):
        p = planner(sizes, 10, env)
        assert {k: p[k] for k in want} == want, env


def test_knob_clamps_and_rounds(planner):
    """Below 256 means 256; 259 rounds down to 256; 300 is taken as it is; on
    the claim path too."""
    sh = SHAPES["K2"]
    at256 = planner(sh.sizes, 10, {"ADL_BLOOM_CHUNK_KEYS": "256"})
    assert at256["C"] == 256
    for v in ("1", "100", "255", "257", "259"):
        assert planner(sh.sizes, 10, {"ADL_BLOOM_CHUNK_KEYS": v}) == at256, v
    assert planner(sh.sizes, 10, {"ADL_BLOOM_CHUNK_KEYS": "300"})["C"] in range(260, 301, 4)
    assert planner(sh.sizes, 10, {"ADL_BLOOM_CHUNK_KEYS": "303"})["C"] in range(260, 301, 4)
    cl = planner(sh.sizes, 10, {"ADL_BLOOM_CHUNK_KEYS": "259", "ADL_BLOOM_CLAIM": "2"})
    assert cl["claim"] and cl["C"] == 256 and cl["chunks"] == at256["chunks"]
    # a workspace of the size the knob's plan asks for: smaller chunks, more table rows
    assert at256["ws"] != planner(sh.sizes, 10, {})["ws"]
