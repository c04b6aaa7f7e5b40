"""The CPU oracle over the router's whole input range (tests/router_ranges.py), against XR-Maze restated in Python integers.

The oracle is what every GPU router form is compared with, and its own arithmetic (uint32 keys, int32 coordinates) had never been run
at a span of 2^31, a penalty of 2^22 - 1 or an edge of exactly XR_DIST_CAP.  Here: for every magnitude class and axis, the distance
field of every net of the initial state equals `distance_field_bigint`, and a whole episode equals `Twin` step by step — status,
deltas (re-derived from the path in Python integers), a contiguous path, owners and the hash chain.

Non-vacuity is asserted on the oracle alone, so that tests/test_gpu_router_ranges.py cannot pass on batches that never exercise what
their class is named after."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import router_ranges as rr

CASES = rr.all_cases()


@functools.lru_cache(maxsize=None)
def oracle_episode(name, axis):
    c = rr.case(name, axis)
    return played(c.regions, c.costs, c.id)


def played(regions, costs, what_id):
    """Every region played to its end on the oracle, lowest legal net first; each step checked against the twin.  Returns per region the
    list of the twin's step records (the oracle's: equal)."""
    from oracle import xr_oracle as orc
    out = []
    for ri, r in enumerate(regions):
        env, tw = orc.OracleEnv(r, **costs), rr.Twin(r, costs)
        steps = []
        while tw.legal:
            assert env.legal().tolist() == tw.legal
            net = tw.legal[0]
            got, want = env.step(net), tw.step(net)
            what = (what_id, ri, net)
            assert got["status"] == want["status"], what
            assert got["delta"].tolist() == want["delta"], what
            assert got["path_len"] == want["path_len"] and got["path"].tolist() == want["path"], what
            assert got["done"] == want["done"] and env.cum().tolist() == tw.cum, what
            assert env.owner().tolist() == tw.owner and env.hash() == tw.hash, what
            steps.append(want)
        assert env.nlegal() == 0
        out.append(steps)
    return out


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_oracle_distance_fields_equal_the_bigint_reference(c):
    from oracle import xr_oracle as orc
    assert 4 <= len(c.regions) <= 8
    for ri, r in enumerate(c.regions):
        assert r.n_nodes <= 600                                   # (cap_region's 300x2x1 is the ceiling)
        env = orc.OracleEnv(r, **c.costs)
        for net in rr.Twin(r, c.costs).legal:
            got = env.distance_field(net)
            want = rr.distance_field_bigint(r, net, c.costs)
            assert got.tolist() == want, (c.id, ri, net)
            reached = [d for d in want if d != rr.INF]
            assert max(reached) < rr.DIST_CAP                     # what exists is below the cap


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_oracle_episode_equals_the_twin_and_the_class_is_not_vacuous(c):
    steps = [s for region in oracle_episode(c.name, c.axis) for s in region]
    assert any(s["path_len"] > 1 for s in steps), "no net of the class is routed over an edge"
    if c.name == "cap_edge" or c.name.startswith("span_"):
        assert any(s["status"] & rr.UNREACHABLE for s in steps) and any(not s["status"] & rr.UNREACHABLE and s["path_len"] > 1 for s in steps)
    if c.name == "unit_beside_wide":                               # a reached target further than 10^6 (of wire: penalties and vias apart)
        assert any(not s["status"] & rr.UNREACHABLE and s["delta"][1] > 10 ** 6 for s in steps)
    if c.name.startswith("step_") or c.name.startswith("pen_max"):
        assert any(s["held"] > 0 for s in steps), "no path crosses a held node: the penalty never enters a distance"
    if c.name == "guide_max":
        assert any(s["outside_guide"] > 0 for s in steps), "no path leaves its guide: guide_cost never enters a distance"
    if c.name.startswith("via_") or c.name == "step_inside_via" or c.name == "step_outside_via":
        assert any(s["delta"][2] > 0 for s in steps), "no path takes a via"


def test_cap_edge_is_reached_at_the_cap_minus_one_and_not_at_the_cap():
    """The bare edge: net 3 of the gap ladders sits on the two tracks that border the gap."""
    from oracle import xr_oracle as orc
    for axis in ("x", "y"):
        c = rr.case("cap_edge", axis)
        below, at = c.regions[0], c.regions[1]
        for r, want in ((below, rr.DIST_CAP - 1), (at, rr.INF)):
            tw = rr.Twin(r, c.costs)
            target = tw.aps[3][1][0]
            assert orc.OracleEnv(r, **c.costs).distance_field(3)[target] == want == rr.distance_field_bigint(r, 3, c.costs)[target]
        four_below, four_at = c.regions[2], c.regions[3]
        for r, want in ((four_below, rr.DIST_CAP - 1), (four_at, rr.INF)):
            target = rr.Twin(r, c.costs).aps[1][1][0]
            assert orc.OracleEnv(r, **c.costs).distance_field(1)[target] == want == rr.distance_field_bigint(r, 1, c.costs)[target]


def test_the_table_places_every_batch_where_its_name_says():
    """The quantities place_route decides on (xr_batch.cpp), recomputed from the regions: each inside / outside pair differs in exactly
    the term it is named after."""
    def extents(c):
        gaps = [int(g) for r in c.regions for g in list(np.diff(r.xs.astype(np.int64))) + list(np.diff(r.ys.astype(np.int64)))]
        ext = max(max(int(r.xs[-1]) - int(r.xs[0]), int(r.ys[-1]) - int(r.ys[0])) for r in c.regions)
        return max(gaps + [c.costs["via_cost"]]), min(gaps + [c.costs["via_cost"]]), ext
    for axis in rr.AXES:
        for t in rr.STEP_TERMS:
            for side, total in (("inside", rr.STEP_LIMIT - 1), ("outside", rr.STEP_LIMIT)):
                c = rr.case(f"step_{side}_{t}", axis)
                e_max, _, ext = extents(c)
                assert e_max + c.pen_max + c.costs["guide_cost"] == total and ext < rr.EXTENT_LIMIT and c.costs["via_cost"] * 32 < rr.EXTENT_LIMIT
        for side, want in (("inside", rr.EXTENT_LIMIT - 1), ("outside", rr.EXTENT_LIMIT)):
            c = rr.case(f"extent_{side}", axis)
            e_max, _, ext = extents(c)
            assert ext == want and e_max + c.pen_max < rr.STEP_LIMIT
        for name, via in (("via_inside", rr.STEP_LIMIT - 1), ("via_outside", rr.STEP_LIMIT), ("via_max", rr.COST_LIMIT - 1)):
            assert rr.case(name, axis).costs["via_cost"] == via
        c = rr.case("via_inside", axis)
        assert extents(c)[0] + c.pen_max < rr.STEP_LIMIT
        c = rr.case("unit_beside_wide", axis)
        e_max, e_min, _ = extents(c)
        assert e_min == 1 and e_max + c.pen_max == rr.STEP_LIMIT - 2
        assert rr.case("pen_max_m1", axis).pen_max == rr.COST_LIMIT - 1 and rr.case("pen_max_m3", axis).pen_max == rr.COST_LIMIT - 4
        assert rr.case("guide_max", axis).costs["guide_cost"] == rr.COST_LIMIT - 1
        for name, span in (("span_inside", rr.SPAN_LIMIT - 1), ("span_2p29", 1 << 29), ("span_2p30", 1 << 30), ("span_2p31", 1 << 31)):
            assert extents(rr.case(name, axis))[2] == span and bool(rr.case(name, axis).refused) == (span >= rr.SPAN_LIMIT)
        lo, hi = rr.case("offset_low", axis), rr.case("offset_high", axis)
        for r_lo, r_hi, r0 in zip(lo.regions, hi.regions, rr.base_regions()):
            if "x" in axis:
                assert int(r_lo.xs[0]) == -rr.COORD_LIMIT and int(r_hi.xs[-1]) == rr.COORD_LIMIT and np.array_equal(np.diff(r_lo.xs), np.diff(r0.xs))
            if "y" in axis:
                assert int(r_lo.ys[0]) == -rr.COORD_LIMIT and int(r_hi.ys[-1]) == rr.COORD_LIMIT and np.array_equal(np.diff(r_hi.ys), np.diff(r0.ys))
            assert np.array_equal(r_lo.nodes, r0.nodes)


def test_offsets_change_nothing_on_the_oracle():
    flat = lambda ep: [(s["status"], s["delta"], s["path"]) for region in ep for s in region]
    base = flat(played(list(rr.base_regions()), rr.DEFAULT_COSTS, "base"))
    for axis in rr.AXES:
        for name in ("offset_low", "offset_high"):
            assert flat(oracle_episode(name, axis)) == base, (name, axis)


def test_oracle_at_a_gap_of_2p31_under_the_sanitizers():
    """tests/hostsan/oracle_span.c: the oracle with ASan + UBSan linked in, as a program of its own, on tracks at -2^30 and +2^30.  The
    int32 difference of those two coordinates overflows (the oracle took edge lengths that way until this table was run); the edge is
    2^31 - 800 DBU >= XR_DIST_CAP, so net 1's second pin is unreachable, and net 2 routes 400 DBU and one via at the high end."""
    hostsan = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsan")
    r = subprocess.run(["make", "-C", hostsan, "oracle_span"], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-1500:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([os.path.join(hostsan, "oracle_span")], capture_output=True, text=True, env=env, timeout=60)
    assert out.returncode == 0 and out.stderr == "", (out.stdout[-500:], out.stderr[-2000:])
    U = str(rr.INF)
    f1 = ["400", "1200"] + [U] * 4 + ["0", "800"] + [U] * 16
    f2 = [U] * 14 + ["0", "800"] + [U] * 4 + ["400", "1200"] + [U] * 2
    assert out.stdout.splitlines() == ["field 1: " + " ".join(f1), "field 2: " + " ".join(f2),
                                       "step 1: status 2 delta 1 0 0 done 0 path", "step 2: status 0 delta 0 400 1 done 1 path 21 20 14"]
