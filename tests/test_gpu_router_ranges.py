"""GPU parity over the router's whole input range: every magnitude class of tests/router_ranges.py (each along x, y and both) under
every router form, whole episodes against the CPU oracle — status, delta, cum, done, path_len, path, owner and the final hash chain,
exactly.  Equal statuses are required, so a spurious XR_ENV_ROUTER_ABORT fails the test.

tests/test_router_ranges_host.py pins the oracle itself on the same table against Python integers and asserts that every class
exercises what it is named after; tests/hostsan/load_trace.cpp pins which router form the loader picks at each threshold.  Here the
inside / outside pairs also check, by the LDS the step kernel asks for, that the GPU run took the form the host trace says.

What the library refuses is asserted, not skipped: XR-Maze v2 knobs with the sweeps, and a track span of 2^28 DBU or more."""
import functools

import numpy as np
import pytest
import torch

from tests import router_ranges as rr

pytestmark = pytest.mark.gpu

FORMS = {
    "default": dict(),                                            # round 3's LDS form inside its limits, round 2's outside
    "lds-round2": dict(router=3),
    "sweeps": dict(router=1),
    "scratch": dict(force_scratch_field=True, window=-1),
    "window": dict(force_scratch_field=True, window=1000),
}
V2_EXTRA = {                                                      # step_* and extent_*: a second attempt at twice the penalty
    "lds-v2": dict(maze_end_iter=2),
    "scratch-v2": dict(maze_end_iter=2, force_scratch_field=True, window=-1),
}
V2_NEEDS_FRONTIER = "XR-Maze v2 (guide_cost / maze_end_iter) needs the frontier router"
CASES = rr.all_cases()


def _costs(c, form):
    return dict(c.costs, **{k: v for k, v in form.items() if k in c.costs})


def _play(regions, costs):
    from oracle import xr_oracle as orc
    out = []
    for r in regions:
        env = orc.OracleEnv(r, **costs)
        steps = []
        while env.nlegal():
            net = int(env.legal()[0])
            res = env.step(net)
            steps.append((net, res, env.cum().copy(), env.owner().copy()))
        out.append((steps, env.hash()))
    return out


@functools.lru_cache(maxsize=None)
def oracle_episode(name, axis, maze_end_iter):
    """The class's regions played to their end on the oracle, lowest legal net first (computed once per class and attempt count, shared
    by every form): per region the list of (net, step result, cum, owner) and the final hash."""
    c = rr.case(name, axis)
    return _play(c.regions, dict(c.costs, maze_end_iter=maze_end_iter))


@functools.lru_cache(maxsize=None)
def base_episode():
    """The generated regions on the tracks they were generated with (origins of a few hundred thousand DBU at most)."""
    return _play(rr.base_regions(), rr.DEFAULT_COSTS)


def make_batch(regions, costs, form):
    from xroute_env_amd.batch import RegionBatch
    kw = {k: v for k, v in form.items() if k not in costs}
    return RegionBatch(regions, device="cuda:0", **costs, **kw)


def run_parity(regions, costs, form, reference):
    """Whole episodes on the GPU against `reference` (oracle_episode's records).  Returns the batch and, per region, its (path, delta) list."""
    batch = make_batch(regions, costs, form)
    batch.reset()
    B = len(regions)
    taken = [[] for _ in range(B)]
    n_steps = max(len(steps) for steps, _ in reference)
    for t in range(n_steps + 1):
        legal = batch.legal_sets()
        for i, (steps, _) in enumerate(reference):
            assert sorted(legal[i]) == sorted(s[0] for s in steps[t:]), (i, t)
        if t == n_steps:
            break
        acts = [steps[t][0] if t < len(steps) else 0 for steps, _ in reference]
        batch.step(torch.tensor(acts, dtype=torch.int32, device="cuda:0"))
        status, delta, cum = (batch.fetch(k).cpu().numpy() for k in ("status", "delta", "cum"))
        done, plen, path, owner = (batch.fetch(k).cpu().numpy() for k in ("done", "path_len", "path", "owner"))
        for i, (steps, _) in enumerate(reference):
            if not acts[i]:
                assert status[i] & 1                   # XR_ENV_BAD_ACTION: the env had finished
                continue
            net, ref, ref_cum, ref_owner = steps[t]
            what = (i, t, net)
            assert status[i] == ref["status"], (what, status[i], ref["status"])
            assert delta[i].tolist() == ref["delta"].tolist(), (what, delta[i], ref["delta"])
            assert cum[i].tolist() == ref_cum.tolist(), what
            assert bool(done[i]) == ref["done"], what
            assert plen[i] == ref["path_len"], (what, plen[i], ref["path_len"])
            assert path[i, :plen[i]].tolist() == ref["path"].tolist(), what
            assert np.array_equal(owner[i, :ref_owner.size], ref_owner), what
            taken[i].append((ref["path"].tolist(), ref["delta"].tolist()))
    hashes = batch.fetch("hash").cpu().numpy().view(np.uint64)
    assert [int(h) for h in hashes] == [h for _, h in reference]
    return batch, taken


def assert_refused(regions, costs, form, fragment):
    from xroute_env_amd import _lib
    with pytest.raises(_lib.XRouteError) as err:
        make_batch(regions, costs, form)
    assert err.value.code == _lib.XR_ERR_RANGE and fragment in str(err.value), str(err.value)


def forms_of(c):
    forms = dict(FORMS)
    if c.name.startswith("step_") or c.name.startswith("extent_"):
        forms.update(V2_EXTRA)
    return forms


PARAMS = [pytest.param(c, f, id=f"{c.id}-{f}") for c in CASES for f in forms_of(c)]


@pytest.mark.parametrize("c,form_name", PARAMS)
def test_every_router_form_equals_the_oracle_over_the_class(c, form_name):
    form = forms_of(c)[form_name]
    costs = _costs(c, form)
    if c.refused:                                                 # a span the loader does not take, whatever the form
        return assert_refused(c.regions, costs, form, c.refused)
    if form_name == "sweeps" and (costs["guide_cost"] > 0 or costs["maze_end_iter"] > 1):
        return assert_refused(c.regions, costs, form, V2_NEEDS_FRONTIER)
    reference = oracle_episode(c.name, c.axis, costs["maze_end_iter"])
    _, taken = run_parity(c.regions, costs, form, reference)
    assert sum(len(t) for t in taken) == sum(len(steps) for steps, _ in reference) >= len(c.regions)
    if c.name.startswith("offset_"):
        # metamorphic, on top of the oracle: moving every track by the same amount changes no path and no delta
        _, origin = run_parity(list(rr.base_regions()), costs, form, base_episode())
        assert taken == origin


@pytest.mark.parametrize("axis", rr.AXES)
@pytest.mark.parametrize("inside,outside", rr.PAIRS, ids=[p[0].replace("_inside", "") for p in rr.PAIRS])
def test_the_batch_outside_a_limit_takes_round_2s_form_and_the_one_inside_does_not(inside, outside, axis):
    """route_occupancy()[1] is the LDS the step kernel asks for: round 3's form (xr_dial3.h) and round 2's (xr_dial.h) lay out
    different tables, so the number tells which one the loader picked."""
    cin, cout = rr.case(inside, axis), rr.case(outside, axis)
    lds_in = make_batch(cin.regions, cin.costs, {}).route_occupancy()[1]
    lds_out = make_batch(cout.regions, cout.costs, {}).route_occupancy()[1]
    lds_out_r2 = make_batch(cout.regions, cout.costs, dict(router=3)).route_occupancy()[1]
    lds_in_r2 = make_batch(cin.regions, cin.costs, dict(router=3)).route_occupancy()[1]
    assert lds_out == lds_out_r2 and lds_in != lds_out
    assert lds_in != lds_in_r2                                    # (inside: asking for round 2's form really changes the form)


@pytest.mark.parametrize("axis", rr.AXES)
def test_one_region_outside_a_limit_moves_the_whole_batch(axis):
    """mixed_batch: the dispatcher decides on the maxima over the batch."""
    c = rr.case("mixed_batch", axis)
    lds = make_batch(c.regions, c.costs, {}).route_occupancy()[1]
    assert lds == make_batch(c.regions, c.costs, dict(router=3)).route_occupancy()[1]
    alone = [c.regions[0], c.regions[2]] * 2                      # the ispd-magnitude regions on their own: round 3's form
    assert make_batch(alone, c.costs, {}).route_occupancy()[1] != make_batch(alone, c.costs, dict(router=3)).route_occupancy()[1]


@pytest.mark.parametrize("axis", ("x", "y"))
def test_the_span_limit_is_refused_with_its_name_and_the_span_below_it_is_taken(axis):
    from xroute_env_amd import _lib
    wide = rr.gap_ladder(span=rr.SPAN_LIMIT)
    below = rr.gap_ladder(span=rr.SPAN_LIMIT - 1)
    if axis == "y":
        wide, below = rr.transposed(wide), rr.transposed(below)
    for form in FORMS.values():
        with pytest.raises(_lib.XRouteError) as err:
            make_batch([below, wide], rr.DEFAULT_COSTS, form)
        assert err.value.code == _lib.XR_ERR_RANGE
        assert f"region 1: tracks span {rr.SPAN_LIMIT} DBU in {axis}, the routers take spans below 2^28 (XR_MAX_TRACK_SPAN)" in str(err.value)
        make_batch([below, below], rr.DEFAULT_COSTS, form)
