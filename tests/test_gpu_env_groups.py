"""Env groups on the MI355X: slots stepped independently, one stream per group, with uneven cadences and no host synchronisation
between enqueues, equal — env by env, at equal env_steps — the lock-step batch (hash chains, metrics, legal sets, region rotation,
observation rows); the CPU oracle replays each env's own action sequence; whole-batch calls after group steps; the vector env's
step_async / step_wait; 4096 ispd18_test1-sized slots in 4 concurrent groups; invalid use refused on a live batch."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from xroute_env_amd import _lib
from xroute_env_amd.batch import RegionBatch
from xroute_env_amd.regions import config_regions, generate_region

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x5EED
FIELDS = ("hash", "cum", "delta", "reward", "done", "legal", "region", "replay", "env_steps", "nlegal")


@pytest.fixture(autouse=True)
def _release_cached_memory():
    """Hand the observation buffers of every test back to the driver: a later test that allocates with torch.empty and compares whole
    rows (bytes past an env's (2+7K)*N included) must not inherit these tests' bytes from the caching allocator."""
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _small_regions(dims=(12, 10, 4), n=5, base=8100):
    return [generate_region(base + i, dims=dims, k_range=(2, 5), net_span=5) for i in range(n)]


def _obs_rows(batch, regions, obs, lo, hi):
    """The meaningful prefix (2+7K)*N of every row of envs [lo, hi) (obs row 0 = env lo)."""
    reg = batch.fetch("region")[lo:hi].cpu().numpy()
    nl = batch.fetch("nlegal")[lo:hi].cpu().numpy()
    o = obs.cpu().numpy()
    return [o[i, :(2 + 7 * int(nl[i])) * regions[int(reg[i])].n_nodes].copy() for i in range(hi - lo)]


def _snap(batch, regions, lo, hi, obs_rows=None):
    d = {k: batch.fetch(k)[lo:hi].cpu().numpy().copy() for k in FIELDS}
    if obs_rows is not None:
        d["obs"] = obs_rows
    return d


def _assert_snap_equal(a, b, what):
    for k in FIELDS:
        assert np.array_equal(a[k], b[k]), (what, k, a[k], b[k])
    if "obs" in a:
        for i, (x, y) in enumerate(zip(a["obs"], b["obs"])):
            assert x.tobytes() == y.tobytes(), (what, "observation row", i)


def _grouped_run(a, obs, mode, cadence, rounds):
    """Group g steps cadence[g] times per round on its own stream; nothing synchronises with the host until the join."""
    cur = torch.cuda.current_stream()
    G = a.n_groups
    streams = [torch.cuda.Stream() for _ in range(G)]
    acts = []
    for g, s in enumerate(streams):
        s.wait_stream(cur)
        lo, hi = a.group_bounds(g)
        with torch.cuda.stream(s):
            acts.append(torch.empty(hi - lo, dtype=torch.int32, device=DEV))
    for _ in range(rounds):
        for k in range(max(cadence)):
            for g in range(G):
                if k >= cadence[g]:
                    continue
                s = streams[g]
                lo, hi = a.group_bounds(g)
                with torch.cuda.stream(s):
                    a.random_actions_group(g, SEED, out=acts[g], stream=s)
                    if mode == "route":
                        a.step_group(g, acts[g], stream=s)
                    else:
                        a.step_group(g, acts[g], obs[lo:hi], inplace=(mode == "inplace"), stream=s)
    for s in streams:
        cur.wait_stream(s)
    return [rounds * c for c in cadence]


def _twin_snaps(b, regions, obs_b, mode, bounds, counts):
    """Lock-step twin: step every env max(counts) times; group g's slice is captured after counts[g] steps."""
    act = torch.empty(b.n_envs, dtype=torch.int32, device=DEV)
    snaps = {}
    for t in range(1, max(counts) + 1):
        b.random_actions(SEED, act)
        if mode == "route":
            b.step(act)
        else:
            b.step(act, obs_b, inplace=(mode == "inplace"))
        for g, c in enumerate(counts):
            if c == t:
                lo, hi = bounds[g], bounds[g + 1]
                if mode == "route":
                    o = b.observation(env_lo=lo, env_hi=hi)
                else:
                    o = obs_b[lo:hi]
                snaps[g] = _snap(b, regions, lo, hi, _obs_rows(b, regions, o, lo, hi))
    return snaps


def _make(regions, n_envs, **kw):
    return RegionBatch(regions, n_envs=n_envs, device=DEV, auto_reset=True, max_route_count=1, **kw)


def _start(batch, obs):
    batch.reset(rotate=True)
    if obs is not None:
        batch.observation(obs)


FORMS = {
    "queue_inplace": ("inplace", {}, (12, 10, 4)),
    "full_write": ("full", {}, (12, 10, 4)),
    "route_only": ("route", {}, (12, 10, 4)),
    "sweeps": ("inplace", dict(router=1), (12, 10, 4)),
    "hbm_scratch": ("inplace", dict(force_scratch_field=True), (12, 10, 4)),
    "maze_v2": ("inplace", dict(guide_cost=500, guide_margin=1, maze_end_iter=3), (12, 10, 4)),
    "stream_per_region": ("full", dict(stream_per_region=True), (12, 10, 4)),
    "unaligned_planes": ("inplace", {}, (7, 9, 5)),
}
PARTITIONS = {"one": [0, 24], "four_equal": [0, 6, 12, 18, 24], "uneven": [0, 1, 7, 24]}


@pytest.mark.parametrize("part", list(PARTITIONS))
@pytest.mark.parametrize("form", list(FORMS))
def test_group_steps_equal_lockstep(form, part):
    mode, kw, dims = FORMS[form]
    bounds = PARTITIONS[part]
    regions = _small_regions(dims)
    n = bounds[-1]
    a, b = _make(regions, n, **kw), _make(regions, n, **kw)
    a.set_groups(bounds)
    obs_a = a.alloc_observation().zero_() if mode != "route" else None
    obs_b = b.alloc_observation().zero_() if mode != "route" else None
    _start(a, obs_a)
    _start(b, obs_b)
    cadence = [g + 1 for g in range(a.n_groups)]
    counts = _grouped_run(a, obs_a, mode, cadence, rounds=8)
    torch.cuda.synchronize()
    snaps_b = _twin_snaps(b, regions, obs_b, mode, bounds, counts)
    for g in range(a.n_groups):
        lo, hi = bounds[g], bounds[g + 1]
        o = a.observation(env_lo=lo, env_hi=hi) if mode == "route" else obs_a[lo:hi]
        sa = _snap(a, regions, lo, hi, _obs_rows(a, regions, o, lo, hi))
        assert (sa["env_steps"] > 0).all()
        _assert_snap_equal(sa, snaps_b[g], (form, part, g))
    # episodes ended, auto-reset and rotated inside the groups
    reg = a.fetch("region").cpu().numpy()
    assert (reg != np.arange(n) % len(regions)).any()


def test_group_steps_vs_oracle():
    from oracle import xr_oracle as orc
    regions = [generate_region(8300 + i, dims=(8, 7, 4), k_range=(2, 5), net_span=4) for i in range(6)]
    batch = RegionBatch(regions, device=DEV)
    batch.set_groups([0, 1, 3, 6])
    envs = [orc.OracleEnv(r) for r in regions]
    batch.reset()
    obs = batch.alloc_observation().zero_()
    steps, rnd = 0, 0
    while any(e.nlegal() for e in envs):
        for g in range(batch.n_groups):
            lo, hi = batch.group_bounds(g)
            for _ in range(1 + (g + rnd) % 3):         # uneven cadence, rotating
                legal = [envs[e].legal().tolist() for e in range(lo, hi)]
                if not any(legal):
                    break
                acts = [max(s) if s else 0 for s in legal]
                batch.step_group(g, torch.tensor(acts, dtype=torch.int32, device=DEV), obs[lo:hi], inplace=(rnd % 2 == 1))
                delta = batch.fetch_group("delta", g).cpu().numpy()
                done = batch.fetch_group("done", g).cpu().numpy()
                plen = batch.fetch_group("path_len", g).cpu().numpy()
                path = batch.fetch_group("path", g).cpu().numpy()
                nleg = batch.fetch_group("nlegal", g).cpu().numpy()
                o = obs[lo:hi].cpu().numpy()
                for i, e in enumerate(range(lo, hi)):
                    if not acts[i]:
                        continue
                    ref = envs[e].step(acts[i])
                    assert ref["delta"].tolist() == delta[i].tolist(), (e, ref["delta"], delta[i])
                    assert ref["done"] == bool(done[i])
                    assert ref["path"].tolist() == path[i, :plen[i]].tolist()
                    ro = envs[e].observation()
                    assert np.array_equal(ro.ravel(), o[i, :ro.size]), ("observation", e)
                    assert nleg[i] == envs[e].nlegal()
                    steps += 1
        rnd += 1
    hashes = batch.fetch("hash").cpu().numpy().view(np.uint64)
    assert [int(h) for h in hashes] == [e.hash() for e in envs]
    assert steps > 10


def test_whole_batch_calls_after_groups():
    regions = _small_regions()
    bounds = [0, 5, 6, 24]
    a, b = _make(regions, 24), _make(regions, 24)
    a.set_groups(bounds)
    obs_a, obs_b = a.alloc_observation().zero_(), b.alloc_observation().zero_()
    _start(a, obs_a)
    _start(b, obs_b)
    # every group steps 5 times, interleaved unevenly in time: equal totals, so the whole batches must match
    cur = torch.cuda.current_stream()
    streams = [torch.cuda.Stream() for _ in range(3)]
    acts = [torch.empty(bounds[g + 1] - bounds[g], dtype=torch.int32, device=DEV) for g in range(3)]
    for s in streams:
        s.wait_stream(cur)
    order = [2, 2, 0, 1, 2, 0, 0, 1, 1, 2, 0, 1, 2, 0, 1]
    for g in order:
        lo, hi = bounds[g], bounds[g + 1]
        with torch.cuda.stream(streams[g]):
            a.random_actions_group(g, SEED, out=acts[g], stream=streams[g])
            a.step_group(g, acts[g], obs_a[lo:hi], inplace=True, stream=streams[g])
    for s in streams:
        cur.wait_stream(s)
    act_b = torch.empty(24, dtype=torch.int32, device=DEV)
    for _ in range(5):
        b.random_actions(SEED, act_b)
        b.step(act_b, obs_b, inplace=True)
    # the in-place buffers, fingerprint, state_dict
    ra, rb = _obs_rows(a, regions, obs_a, 0, 24), _obs_rows(b, regions, obs_b, 0, 24)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ra, rb))
    assert a.fingerprint() == b.fingerprint()
    da, db = a.state_dict(), b.state_dict()
    for k in a._STATE:
        assert torch.equal(da[k], db[k]), k
    # the first whole-batch in-place call after group steps writes everything (and equals the twin's in-place result)
    act_a = torch.empty(24, dtype=torch.int32, device=DEV)
    a.random_actions(SEED, act_a)
    b.random_actions(SEED, act_b)
    assert torch.equal(act_a, act_b)
    a.step(act_a, obs_a, inplace=True)
    assert not a.observe_info()["inplace"]
    b.step(act_b, obs_b, inplace=True)
    assert b.observe_info()["inplace"]
    ra, rb = _obs_rows(a, regions, obs_a, 0, 24), _obs_rows(b, regions, obs_b, 0, 24)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ra, rb))
    a.step(act_a, obs_a, inplace=True)          # and the next one is in place again
    assert a.observe_info()["inplace"]
    b.step(act_a, obs_b, inplace=True)
    # one group: today's behaviour
    a.set_groups([0, 24])
    assert a.n_groups == 1
    with pytest.raises(_lib.XRouteError) as ei:
        _lib.check(a.L.xr_batch_step_group(a._h, 1, C.c_void_p(act_a.data_ptr()), None, 0, 0, None))
    assert ei.value.code == _lib.XR_ERR_RANGE
    a.random_actions(SEED, act_a)
    b.random_actions(SEED, act_b)
    a.step(act_a, obs_a, inplace=True)
    b.step(act_b, obs_b, inplace=True)
    assert a.observe_info()["inplace"]
    for k in FIELDS:
        assert torch.equal(a.fetch(k), b.fetch(k)), k
    ra, rb = _obs_rows(a, regions, obs_a, 0, 24), _obs_rows(b, regions, obs_b, 0, 24)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ra, rb))
    # xr_batch_observation into fresh buffers (last: it moves the batch's in-place buffer)
    ra, rb = _obs_rows(a, regions, a.observation(), 0, 24), _obs_rows(b, regions, b.observation(), 0, 24)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ra, rb))


def _env_pair(dict_observation=False, groups=4):
    from xroute_env_amd.envs import XRouteVectorEnv
    regions = _small_regions()
    ea = XRouteVectorEnv(regions, n_envs=24, device=DEV, groups=groups, dict_observation=dict_observation)
    eb = XRouteVectorEnv(regions, n_envs=24, device=DEV, dict_observation=dict_observation)
    return ea, eb


def _same_step(ra, rb):
    oa, rwa, da, ia = ra
    ob, rwb, db, ib = rb
    if isinstance(oa, dict):
        assert set(oa) == set(ob) == {"grid", "legal_mask"}
        for k in oa:
            assert torch.equal(oa[k], ob[k]), k
    else:
        assert torch.equal(oa, ob)
    assert torch.equal(rwa, rwb) and torch.equal(da, db)
    assert set(ia) == set(ib)
    for k in ia:
        assert torch.equal(ia[k], ib[k]), k


def test_vector_env_step_async_wait():
    for dict_obs in (False, True):
        ea, eb = _env_pair(dict_observation=dict_obs)
        oa, _ = ea.reset()
        ob, _ = eb.reset()
        assert ea.n_groups == 4 and len(ea.group_streams) == 4
        for _ in range(12):
            acts = eb.random_actions(SEED)
            ea.step_async(acts.clone())
            ra = ea.step_wait()
            rb = eb.step(acts)
            _same_step(ra, rb)
            if dict_obs:
                assert ra[0]["grid"].data_ptr() == ea.obs.data_ptr()
    # per-group poll / ready_groups loop: a group steps again as soon as its last step has finished
    ea, eb = _env_pair(groups=[0, 1, 7, 24])
    ea.reset()
    eb.reset()
    K = 10
    done = [0] * ea.n_groups
    while min(done) < K:
        ready = ea.ready_groups()
        assert all(ea.poll(g) for g in ready)
        for g in ready:
            if done[g] >= K:
                continue
            if done[g] > 0:
                o, r, d, info = ea.step_wait(g)
                lo, hi = ea.batch.group_bounds(g)
                assert o.shape[0] == hi - lo and r.shape == (hi - lo,) and info["legal"].shape[0] == hi - lo
            s = ea.group_streams[g]
            with torch.cuda.stream(s):
                acts = ea.batch.random_actions_group(g, SEED, stream=s)
            ea.step_async(acts, group=g)
            done[g] += 1
    ra = ea.step_wait()
    torch.cuda.synchronize()
    assert ea.ready_groups() == list(range(ea.n_groups))
    for _ in range(K):
        rb = eb.step(eb.random_actions(SEED))
    _same_step(ra, rb)
    # a whole-batch step() after group work joins it first
    acts = eb.random_actions(SEED)
    _same_step(ea.step(acts.clone()), eb.step(acts))


def test_concurrent_groups_at_scale():
    regions = config_regions(4, 64)
    n = 4096
    bounds = [0, 1024, 2048, 3072, 4096]
    a, b = _make(regions, n), _make(regions, n)
    a.set_groups(bounds)
    obs_a, obs_b = a.alloc_observation().zero_(), b.alloc_observation().zero_()
    _start(a, obs_a)
    _start(b, obs_b)
    cadence = [1, 3, 2, 4]
    rounds = 12
    counts = _grouped_run(a, obs_a, "inplace", cadence, rounds)
    torch.cuda.synchronize()
    act = torch.empty(n, dtype=torch.int32, device=DEV)
    snaps = {}
    for t in range(1, max(counts) + 1):
        b.random_actions(SEED, act)
        b.step(act, obs_b, inplace=True)
        for g, c in enumerate(counts):
            if c == t:
                snaps[g] = {k: b.fetch(k)[bounds[g]:bounds[g + 1]].cpu().numpy() for k in ("hash", "env_steps", "cum", "region")}
    for g in range(4):
        lo, hi = bounds[g], bounds[g + 1]
        for k in ("hash", "env_steps", "cum", "region"):
            assert np.array_equal(a.fetch(k)[lo:hi].cpu().numpy(), snaps[g][k]), (g, k)
    steps = a.fetch("env_steps")
    assert int(steps[3072:].min()) > int(steps[:1024].max())          # the groups really did progress unevenly


def test_invalid_group_use_on_a_live_batch():
    regions = _small_regions()
    a, b = _make(regions, 24), _make(regions, 24)
    a.set_groups([0, 10, 24])
    _start(a, None)
    _start(b, None)
    L, h = a.L, a._h
    act = torch.ones(24, dtype=torch.int32, device=DEV)
    p = C.c_void_p(act.data_ptr())

    def codes(*bounds_list):
        out = []
        for bl in bounds_list:
            arr = np.ascontiguousarray(bl, np.int32)
            out.append(L.xr_batch_set_groups(h, arr.ctypes.data, arr.size - 1))
        return out
    assert codes([0, 24, 24], [1, 24], [0, 12, 11, 24], [0, 25], [0, 23]) == [_lib.XR_ERR_INVALID] * 5
    arr = np.arange(66, dtype=np.int32)
    assert L.xr_batch_set_groups(h, arr.ctypes.data, 65) == _lib.XR_ERR_RANGE
    assert L.xr_batch_set_groups(h, arr.ctypes.data, 0) == _lib.XR_ERR_RANGE
    assert a.n_groups == 2              # refused partitions leave the one in force
    for g in (-1, 2, 1000):
        assert L.xr_batch_step_group(h, g, p, None, 0, 0, None) == _lib.XR_ERR_RANGE
        assert L.xr_batch_random_actions_group(h, g, p, 1, None) == _lib.XR_ERR_RANGE
        assert L.xr_batch_fetch_group(h, g, _lib.XR_FETCH_HASH, p, 80, None) == _lib.XR_ERR_RANGE
    buf = torch.empty(1024, dtype=torch.uint8, device=DEV)
    q = C.c_void_p(buf.data_ptr())
    assert L.xr_batch_fetch_group(h, 0, _lib.XR_FETCH_HASH, q, 79, None) == _lib.XR_ERR_RANGE
    assert L.xr_batch_fetch_group(h, 0, _lib.XR_FETCH_HASH, q, 81, None) == _lib.XR_ERR_RANGE
    for sel in (_lib.XR_FETCH_STEPS, _lib.XR_FETCH_UNITS, _lib.XR_FETCH_ROUTE_ORDER):
        assert L.xr_batch_fetch_group(h, 0, sel, q, 8, None) == _lib.XR_ERR_INVALID
    assert L.xr_batch_step_group(h, 0, p, None, 0, 2, None) == _lib.XR_ERR_INVALID
    with pytest.raises(ValueError):
        a.step_group(0, act)                      # 24 actions for a group of 10
    # the batch is still usable and still equals its twin
    acts_b = torch.empty(24, dtype=torch.int32, device=DEV)
    for _ in range(4):
        for g in range(2):
            a.step_group(g, a.random_actions_group(g, SEED))
        b.step(b.random_actions(SEED, acts_b))
    for k in FIELDS:
        assert torch.equal(a.fetch(k), b.fetch(k)), k
