"""Branch on the MI355X (xr_batch_branch / RegionBatch.branch / XRouteVectorEnv.branch) and beam search on top of it: gather semantics
against the state before the call for every kind of map (swaps, cycles, chains, fan-outs from overwritten slots, non-injective maps,
pairs across regions); a branched slot is a working env (a twin restored through load_state_dict, and the CPU oracle); out-of-range
parents; done slots and auto-reset; env groups on their own streams; the in-place observation buffers; every router variant; lookahead
and rollouts after a branch; errors; beam search against the greedy episode, the oracle and prefix rollouts; 4096 ispd18_test1 slots."""
import ctypes as C
import gc
import os

import numpy as np
import pytest
import torch

from xroute_env_amd import _lib
from xroute_env_amd.batch import RegionBatch
from xroute_env_amd.regions import generate_region

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0xB4A7
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAD = _lib.XR_ENV_BAD_ACTION
M64 = 2 ** 64 - 1
# every per-env array xr_batch_fetch returns: what a branch moves
ROWS = ("owner", "legal", "nlegal", "cum", "delta", "reward", "done", "status", "path", "path_len", "hash", "region", "replay",
        "env_steps", "record", "sweeps", "touched")
# what the twin (restored through load_state_dict, which does not carry path / sweeps / touched) is compared on
TWIN_ROWS = ("record", "hash", "legal", "owner", "nlegal", "cum", "delta", "reward", "done", "status", "path_len", "region", "replay", "env_steps")


@pytest.fixture(autouse=True)
def _release_cached_memory():
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _pack(sl=slice(None)):
    from xroute_env_amd.lefdef import load_region_pack
    return load_region_pack(os.path.join(GOLDEN, "ispd18_test1_regions.npz"))[sl]


_MIXED = []


def _mixed_regions():
    """The small mixed set of the rollout tests: regions of different sizes, one with N % 8 != 0 (13 x 17 x 4)."""
    if not _MIXED:
        from tests.helpers import obs_set_regions
        extra = [generate_region(9100 + i, dims=d, k_range=(4, 10), pins=(3, 5), net_span=7)
                 for i, d in enumerate([(16, 12, 5), (20, 14, 6), (13, 17, 4), (24, 20, 5)])]
        _MIXED.extend(obs_set_regions("mixed") + extra)
    return list(_MIXED)


def _snap(b, keys=ROWS):
    d = {k: b.fetch(k).cpu().numpy() for k in keys}
    d["steps"] = b.fetch("steps").cpu().numpy()
    return d


def _snap_all(b):
    """Every array xr_batch_fetch returns, as bytes."""
    return {k: b.fetch(k).cpu().numpy().tobytes() for k in b._FETCH}


def _advance(b, steps, history=None, start=0, stagger=True):
    """Seeded random steps; with `stagger` env e sits out the steps whose number is >= 1 + e % (steps + 1) (action 0: a flagged no-op),
    so that slots differ in nets left, cum, hash and env_steps.  history[e] collects the nets env e routed."""
    n = b.n_envs
    e = torch.arange(n, device=DEV)
    for i in range(start, start + steps):
        act = b.random_actions(SEED + 1000 + i)
        if stagger:
            act = torch.where(i - start < 1 + e % (steps + 1), act, torch.zeros_like(act)).contiguous()
        b.step(act)
        if history is not None:
            for k, a in enumerate(act.cpu().numpy().tolist()):
                if a:
                    history[k].append(a)


def _advanced(regions, n, steps=4, **kw):
    b = RegionBatch(regions, n_envs=n, device=DEV, **kw)
    b.reset()
    history = [[] for _ in range(n)]
    _advance(b, steps, history)
    return b, history


def _resolve(parent, rows):
    """Where every row's state comes from, and which rows are flagged."""
    p = np.asarray(parent, np.int64)
    i = np.arange(rows)
    flagged = p >= rows
    return np.where((p < 0) | flagged, i, p), flagged


def _expected(before, src, flagged):
    want = {k: before[k][src].copy() for k in ROWS}
    want["status"][flagged] |= BAD
    rec = want["record"].view(np.uint16)          # status: the last 16 bits of the 48-byte record
    rec[flagged, 23] |= BAD
    return want


def _assert_gathered(b, before, parent, what=""):
    src, flagged = _resolve(parent, b.n_envs)
    after = _snap(b)
    want = _expected(before, src, flagged)
    for k in ROWS:
        assert after[k].tobytes() == want[k].tobytes(), (what, k, np.flatnonzero((after[k] != want[k]).reshape(b.n_envs, -1).any(1))[:8])
    assert after["steps"].tobytes() == before["steps"].tobytes(), what
    return src


def _branch(b, parent, **kw):
    b.branch(torch.tensor(np.asarray(parent, np.int64).astype(np.int32), dtype=torch.int32, device=DEV), **kw)


def _twin_of(regions, n, sd, src, **kw):
    """A fresh batch brought to `sd` indexed by `src` through load_state_dict: the route a caller had before branch existed."""
    t = RegionBatch(regions, n_envs=n, device=DEV, **kw)
    t.reset()
    idx = torch.as_tensor(np.asarray(src, np.int64))
    d = {k: (v if k.startswith("_") or k == "steps" else v[idx].contiguous()) for k, v in sd.items()}
    t.load_state_dict(d)
    return t


def _step_both(a, t, steps, seed, later=None, what=""):
    """`steps` random steps of both batches, each under its own random_actions: the actions and then every compared row must agree."""
    for s in range(steps):
        act_a, act_t = a.random_actions(seed + s), t.random_actions(seed + s)
        assert torch.equal(act_a, act_t), (what, s)
        a.step(act_a); t.step(act_t)
        if later is not None:
            for e, v in enumerate(act_a.cpu().numpy().tolist()):
                if v:
                    later[e].append(v)
        sa, st = _snap(a, TWIN_ROWS), _snap(t, TWIN_ROWS)
        for k in TWIN_ROWS + ("steps",):
            assert sa[k].tobytes() == st[k].tobytes(), (what, s, k)


def _maps(n, rng):
    i = np.arange(n)
    swap = i ^ 1
    cyc = i.copy(); cyc[[3, 7, 11]] = [7, 11, 3]
    chain = (i + 1); chain[-1] = -1
    fan = np.full(n, -1); fan[[1, 2, 4, 5]] = [2, 3, 2, 2]
    cross = np.full(n, -1); cross[0::2] = i[0::2] + 1; cross[1::2] = i[1::2] - 1          # neighbours play different regions
    cross2 = np.full(n, -1); cross2[: n // 2] = i[: n // 2] + n // 2                       # the far half: other regions, other sizes
    return {"identity": i, "all -1": np.full(n, -1), "fan-out of one keeper": np.full(n, 5), "swaps of neighbours": swap, "3-cycle": cyc,
            "chain": chain, "fan-out from an overwritten slot": fan, "permutation": rng.permutation(n),
            "non-injective": rng.integers(0, n, n), "pairs across regions": cross, "far pairs across regions": cross2}


# ---- 1. gather, against the state before -------------------------------------------------------------------------------------------------
MAP_NAMES = ("identity", "all -1", "fan-out of one keeper", "swaps of neighbours", "3-cycle", "chain", "fan-out from an overwritten slot",
             "permutation", "non-injective", "pairs across regions", "far pairs across regions")


@pytest.mark.parametrize("name", MAP_NAMES)
def test_every_map_gathers_from_the_state_before_the_call(name):
    regions = _mixed_regions()
    n = 36
    b, _ = _advanced(regions, n)
    before = _snap(b)
    assert len(set(before["region"].tolist())) == len(regions) and len(set(before["env_steps"].tolist())) > 2
    assert len(set(before["hash"].tolist())) > n // 2 and len(set(before["nlegal"].tolist())) > 2
    assert any(regions[r].n_nodes % 8 for r in before["region"])
    maps = _maps(n, np.random.default_rng(SEED))
    assert tuple(maps) == MAP_NAMES
    parent = maps[name]
    _branch(b, parent)
    src = _assert_gathered(b, before, parent, name)
    moved = src != np.arange(n)
    assert moved.any() == (name not in ("identity", "all -1"))
    if name.endswith("across regions"):
        assert (before["region"][src][moved] != before["region"][moved]).all(), name
    if name == "chain":
        assert moved.sum() == n - 1
    b.step(b.random_actions(SEED))                 # still usable


# ---- 2. a branched slot is a working env -------------------------------------------------------------------------------------------------
def test_a_branched_slot_steps_like_its_parent_would_have():
    from oracle import xr_oracle as orc
    regions = _mixed_regions()
    n = 36
    b, history = _advanced(regions, n)
    rng = np.random.default_rng(SEED + 2)
    parent = rng.integers(0, n, n)
    parent[::5] = -1
    sd = b.state_dict()
    before = _snap(b)
    _branch(b, parent)
    src = _assert_gathered(b, before, parent)
    assert len(set(src.tolist())) < n and (before["region"][src] != before["region"]).any()      # non-injective, across regions
    t = _twin_of(regions, n, sd, src)
    later = [[] for _ in range(n)]
    _step_both(b, t, 3, SEED + 50, later)
    hsh, cum, reg = b.fetch("hash").cpu().numpy().view(np.uint64), b.fetch("cum").cpu().numpy(), b.fetch("region").cpu().numpy()
    checked = 0
    for e in list(np.flatnonzero(src != np.arange(n))[:5]) + [0]:
        env = orc.OracleEnv(regions[int(reg[e])])
        env.reset()
        for a in history[int(src[e])] + later[e]:
            assert not env.step(a)["status"] & BAD
        assert int(hsh[e]) == env.hash() & M64 and cum[e].tolist() == list(env.cum()), e
        checked += 1
    assert checked == 6
    t.close()


# ---- 3. out-of-range parents -------------------------------------------------------------------------------------------------------------
def test_out_of_range_parents_are_flagged_and_keep_their_state():
    regions = _mixed_regions()
    n = 36
    b, _ = _advanced(regions, n)
    rng = np.random.default_rng(SEED + 3)
    parent = rng.integers(0, n, n)
    parent[[4, 9, 20]] = [n, 2 ** 31 - 1, n + 5]
    parent[[5, 6]] = [4, 9]                       # children of flagged slots see them without the flag
    before = _snap(b)
    _branch(b, parent)
    _, flagged = _resolve(parent, n)
    assert flagged.sum() == 3
    _assert_gathered(b, before, parent)
    after = _snap(b)
    assert (after["status"][[4, 9, 20]] & BAD).all() and (after["record"].view(np.uint16)[[4, 9, 20], 23] & BAD).all()
    assert after["status"][5] == before["status"][4] and after["status"][6] == before["status"][9]


# ---- 4. done slots and auto-reset --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("auto_reset", [False, True])
def test_done_and_live_slots_trade_places(auto_reset):
    regions = _mixed_regions()
    n = 24
    kw = dict(auto_reset=auto_reset, max_route_count=1)
    b = RegionBatch(regions, n_envs=n, device=DEV, **kw)
    b.reset()
    for i in range(12):          # until some slots are done and some are not (without letting an auto-reset revive them)
        nl = b.fetch("nlegal").cpu().numpy()
        if (nl == 0).any() and (nl > 0).any():
            break
        b.step(b.random_actions(SEED + i))
    nl = b.fetch("nlegal").cpu().numpy()
    done, live = np.flatnonzero(nl == 0), np.flatnonzero(nl > 0)
    assert done.size and live.size
    k = min(done.size, live.size, 4)
    parent = np.full(n, -1)
    parent[live[:k]] = done[:k]                   # a done slot onto a live one
    parent[done[:k]] = live[:k]                   # and the reverse
    sd = b.state_dict()
    before = _snap(b)
    assert before["done"][done].all()
    _branch(b, parent)
    src = _assert_gathered(b, before, parent)
    t = _twin_of(regions, n, sd, src, **kw)
    _step_both(b, t, 3, SEED + 70, what=auto_reset)
    t.close()


# ---- 5. groups ---------------------------------------------------------------------------------------------------------------------------
def test_a_group_branches_on_its_own_stream_while_another_steps():
    regions = _mixed_regions()
    n = 36
    a, _ = _advanced(regions, n)
    t, _ = _advanced(regions, n)
    a.set_groups(3); t.set_groups(3)
    lo, hi = a.group_bounds(1)
    rows = hi - lo
    rng = np.random.default_rng(SEED + 5)
    parent = rng.integers(0, rows, rows)
    parent[2] = rows + 3                           # valid for the batch, outside the group: flagged, not followed
    parent[3] = n - 1
    parent[4] = -1
    before = _snap(a)
    torch.cuda.synchronize()
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        _branch(a, parent, group=1, stream=s1)
    with torch.cuda.stream(s0):
        a.step_group(0, a.random_actions_group(0, SEED + 9, stream=s0), stream=s0)
    t.step_group(0, t.random_actions_group(0, SEED + 9))
    torch.cuda.synchronize()
    after, twin = _snap(a), _snap(t)
    src, flagged = _resolve(parent, rows)
    assert flagged.tolist() == [i in (2, 3) for i in range(rows)]
    want = _expected({k: before[k][lo:hi] for k in ROWS}, src, flagged)
    for k in ROWS:
        assert after[k][lo:hi].tobytes() == want[k].tobytes(), ("group 1", k)
        assert after[k][:lo].tobytes() == twin[k][:lo].tobytes(), ("group 0", k)
        assert after[k][hi:].tobytes() == twin[k][hi:].tobytes() == before[k][hi:].tobytes(), ("group 2", k)
    assert after["steps"].tobytes() == twin["steps"].tobytes()
    with pytest.raises(ValueError):
        a.branch(torch.zeros(n, dtype=torch.int32, device=DEV), group=1)
    t.close()


# ---- 6. in-place observations ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["batch", "group, then a batch step", "group, then group steps"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])
def test_a_branch_drops_the_in_place_observation_validity(dtype, mode):
    from tests.helpers import SENTINEL_F32, SENTINEL_U8, assert_rows_match_oracle
    regions = _mixed_regions()
    n = 24
    sentinel = SENTINEL_F32 if dtype == torch.float32 else SENTINEL_U8
    grouped = mode != "batch"

    def prepared():
        b = RegionBatch(regions, n_envs=n, device=DEV)
        if grouped:
            b.set_groups(3)
        b.reset()
        buf = b.alloc_observation(dtype=dtype).fill_(sentinel)
        b.step(b.random_actions(SEED + 1), buf)                              # full write: the buffer is valid for the batch and every group
        b.step(b.random_actions(SEED + 2), buf, inplace=True)
        return b, buf

    def step(b, buf, inplace, seed):
        if mode == "group, then group steps":
            for g in range(3):
                lo, hi = b.group_bounds(g)
                b.step_group(g, b.random_actions_group(g, seed), buf[lo:hi], inplace=inplace)
        else:
            b.step(b.random_actions(seed), buf, inplace=inplace)

    a, buf_a = prepared()
    t, buf_t = prepared()
    assert torch.equal(buf_a, buf_t)
    rng = np.random.default_rng(SEED + 6)
    sd = a.state_dict()
    if grouped:
        lo, hi = a.group_bounds(1)
        parent = rng.integers(0, hi - lo, hi - lo)
        _branch(a, parent, group=1)
        src = np.arange(n)
        src[lo:hi] = lo + parent
    else:
        parent = rng.integers(0, n, n)
        _branch(a, parent)
        src = parent
    assert (a.fetch("region").cpu().numpy() != sd["region"].numpy()).any()           # slots changed region: stale net planes would show
    t.load_state_dict({k: (v if k.startswith("_") or k == "steps" else v[torch.as_tensor(src)].contiguous()) for k, v in sd.items()})
    step(a, buf_a, True, SEED + 3)                                                    # in place, as a caller who holds the buffer would
    step(t, buf_t, False, SEED + 3)                                                   # the twin: a full write of the same state
    assert a.fetch("hash").cpu().numpy().tobytes() == t.fetch("hash").cpu().numpy().tobytes()
    assert torch.equal(buf_a, buf_t), mode
    assert_rows_match_oracle(a, buf_a, 0, n, sentinel, full_write=False, what=mode)
    step(a, buf_a, True, SEED + 4)                                                    # and the buffer is valid again afterwards
    step(t, buf_t, False, SEED + 4)
    assert torch.equal(buf_a, buf_t), mode
    assert_rows_match_oracle(a, buf_a, 0, n, sentinel, full_write=False, what=mode)
    t.close()


# ---- 7. variants -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["auto", "dial_r2", "sweep", "v2_guides", "force_scratch_field", "stream_per_region"])
def test_branch_under_every_router_variant(variant):
    if variant == "v2_guides":
        regions = _pack(slice(5, 200, 13))[:12]
        assert all(r.guide_off is not None and r.guide_off[-1] > 0 for r in regions)
        kw = dict(guide_cost=1000, guide_margin=1, maze_end_iter=3)
    elif variant in ("force_scratch_field", "stream_per_region"):
        regions = [generate_region(3000 + i, dims=(12, 10, 4), k_range=(3, 6)) for i in range(4)] + _mixed_regions()[8:10]
        kw = {variant: True}
    else:
        regions = _mixed_regions()
        kw = dict(router={"auto": 0, "sweep": 1, "dial_r2": 3}[variant])
    n = 2 * len(regions)
    b, _ = _advanced(regions, n, steps=3, **kw)
    rng = np.random.default_rng(SEED + 7)
    chain = np.arange(n) + 1; chain[-1] = -1
    for name, parent in (("chain", chain), ("non-injective", rng.integers(0, n, n))):
        sd = b.state_dict()
        before = _snap(b)
        _branch(b, parent)
        src = _assert_gathered(b, before, parent, (variant, name))
        t = _twin_of(regions, n, sd, src, **kw)
        _step_both(b, t, 2, SEED + 80, what=(variant, name))
        t.close()


# ---- 8. queries after a branch -----------------------------------------------------------------------------------------------------------
def test_lookahead_and_rollouts_of_a_branched_slot_equal_its_parents():
    regions = _mixed_regions()
    n = 36
    b, _ = _advanced(regions, n, steps=2)
    words = b.fetch("legal").cpu().numpy().view(np.uint64)
    prefix = np.zeros((n, 2, 2), np.int32)
    for e in range(n):
        nets = [w * 64 + k + 1 for w in range(words.shape[1]) for k in range(64) if (int(words[e, w]) >> k) & 1]
        prefix[e, 0, :len(nets[:2])] = nets[:2]
        prefix[e, 1, :len(nets[-2:])] = nets[-2:][::-1]
    look0, reward0 = (v.cpu().numpy() for v in b.lookahead())
    roll0 = {k: v.cpu().numpy() for k, v in b.rollout(2, policy="stop", prefix=torch.as_tensor(prefix, device=DEV)).items()}
    rng = np.random.default_rng(SEED + 8)
    parent = rng.integers(0, n, n)
    before = _snap(b)
    _branch(b, parent)
    src = _assert_gathered(b, before, parent)
    look1, reward1 = (v.cpu().numpy() for v in b.lookahead())
    assert np.array_equal(look1, look0[src]) and reward1.tobytes() == reward0[src].tobytes()
    roll1 = b.rollout(2, policy="stop", prefix=torch.as_tensor(np.ascontiguousarray(prefix[src]), device=DEV))
    for k, v in roll1.items():
        assert v.cpu().numpy().tobytes() == roll0[k][src].tobytes(), k
    assert (roll0["out"][:, :, 4] > 0).any()
    _assert_gathered(b, before, parent, "the queries left no trace")


# ---- 9. errors ---------------------------------------------------------------------------------------------------------------------------
def test_branch_errors_on_a_live_batch_leave_it_untouched():
    regions = _mixed_regions()[:4]
    b, _ = _advanced(regions, 8, steps=2)
    b.set_groups(2)
    parent = torch.arange(8, dtype=torch.int32, device=DEV).flip(0).contiguous()
    p = C.c_void_p(parent.data_ptr())
    before = _snap_all(b)
    L = b.L
    for args, word in (((b._h, -1, None, None), b"null"), ((None, -1, p, None), b"null"), ((b._h, 2, p, None), b"group"),
                       ((b._h, -2, p, None), b"group"), ((b._h, 64, p, None), b"group")):
        assert L.xr_batch_branch(*args) == _lib.XR_ERR_INVALID, args
        msg = L.xr_last_error()
        assert b"xr_batch_branch" in msg and word in msg, (args, msg)
    fresh = C.c_void_p()
    cfg = _lib.default_config()
    cfg.n_envs = 8
    _lib.check(L.xr_batch_create(C.byref(cfg), C.byref(fresh)))
    assert L.xr_batch_branch(fresh, -1, p, None) == _lib.XR_ERR_STATE and b"load regions first" in L.xr_last_error()
    L.xr_batch_destroy(fresh)
    epoch = b.region_epoch
    for bad in (parent.to(torch.int64), parent[:7].contiguous(), parent.cpu(), torch.arange(16, dtype=torch.int32, device=DEV)[::2]):
        with pytest.raises(ValueError):
            b.branch(bad)
    with pytest.raises(ValueError):
        b.branch(parent, group=2)
    torch.cuda.synchronize()
    assert _snap_all(b) == before and b.region_epoch == epoch
    b.branch(parent)                               # still usable
    assert b.region_epoch == epoch + 1
    b.step(b.random_actions(SEED))


# ---- 10. beam search ---------------------------------------------------------------------------------------------------------------------
def _beam_regions():
    return [generate_region(3000 + i, dims=(12, 10, 4), k_range=(3, 6)) for i in range(4)] + _mixed_regions()[8:10]


def test_beam_of_width_one_is_the_greedy_episode():
    from xroute_env_amd.envs.beam import beam_search
    from xroute_env_amd.envs.vector_env import XRouteVectorEnv
    regions = _beam_regions()
    R = len(regions)
    b = RegionBatch(regions, n_envs=R, device=DEV, auto_reset=False)
    b.assign(list(range(R)))
    b.reset()
    order, ret = [[] for _ in range(R)], np.zeros(R, np.float64)
    for _ in range(b.k_max + 1):
        act = XRouteVectorEnv._argmax_first(b.lookahead()[1])
        a = act.cpu().numpy()
        if not a.any():
            break
        b.step(act)
        rec = b.records()
        for e in np.flatnonzero(a):
            order[e].append(int(a[e]))
            ret[e] = ret[e] + rec["reward"][e]
    res = beam_search(regions, 1, device=DEV)
    assert len(res) == R
    for r in range(R):
        assert len(res[r]) == 1 and res[r][0]["order"] == order[r] and len(order[r]) > 0, r
        assert np.float64(res[r][0]["ret"]).tobytes() == ret[r].tobytes(), r


def test_every_beam_replays_on_the_oracle_and_as_a_prefix_rollout():
    from oracle import xr_oracle as orc
    from xroute_env_amd.envs.beam import beam_search
    regions = _beam_regions()
    R, W = len(regions), 4
    res = beam_search(regions, W, device=DEV)
    again = beam_search(regions, W, device=DEV)
    assert res == again                                                    # two runs: identical results
    assert len(res) == R and all(1 <= len(beams) <= W for beams in res) and any(len(beams) == W for beams in res)
    b = RegionBatch(regions, n_envs=R * W, device=DEV, auto_reset=False)
    b.assign([r for r in range(R) for _ in range(W)])
    b.reset()
    prefix = np.zeros((R * W, 1, max(b.k_max, 1)), np.int32)
    for r, beams in enumerate(res):
        rets = [bm["ret"] for bm in beams]
        assert rets == sorted(rets, reverse=True), r                       # best first
        assert len(set(tuple(bm["order"]) for bm in beams)) == len(beams), r
        for j, bm in enumerate(beams):
            prefix[r * W + j, 0, :len(bm["order"])] = bm["order"]
            env = orc.OracleEnv(regions[r])
            env.reset()
            c0 = np.array(env.cum())
            st, tot = 0, 0.0
            for a in bm["order"]:
                ref = env.step(a)
                assert not ref["status"] & BAD, (r, j, a)
                st |= ref["status"]
                tot = tot + orc.reward(*[int(v) for v in ref["delta"]])
            assert env.nlegal() == 0, (r, j)
            assert bm["delta"] == (np.array(env.cum()) - c0).tolist() and bm["status"] == st, (r, j)
            assert np.float64(bm["ret"]).tobytes() == np.float64(tot).tobytes(), (r, j)
    roll = {k: v.cpu().numpy() for k, v in b.rollout(1, policy="stop", prefix=torch.as_tensor(prefix, device=DEV)).items()}
    for r, beams in enumerate(res):
        for j, bm in enumerate(beams):
            e = r * W + j
            assert roll["out"][e, 0, :3].tolist() == bm["delta"] and int(roll["out"][e, 0, 3]) == bm["status"], (r, j)
            assert int(roll["out"][e, 0, 4]) == len(bm["order"]) and int(roll["out"][e, 0, 5]) == 0, (r, j)
            assert roll["ret"][e, 0].tobytes() == np.float64(bm["ret"]).tobytes(), (r, j)


# ---- 11. full size -----------------------------------------------------------------------------------------------------------------------
def test_branch_at_4096_ispd18_slots():
    regions = _pack()
    n = 4096
    b = RegionBatch(regions, n_envs=n, device=DEV, auto_reset=False)
    b.reset()
    _advance(b, 3)
    rng = np.random.default_rng(SEED + 11)
    parent = rng.integers(0, n, n)
    sd = b.state_dict()
    before = _snap(b)
    _branch(b, parent)
    src = _assert_gathered(b, before, parent, "4096 slots")
    assert (src != np.arange(n)).sum() > n - 8 and len(set(src.tolist())) < n
    t = _twin_of(regions, n, sd, src, auto_reset=False)
    _step_both(b, t, 3, SEED + 90, what="4096 slots")
    t.close()


# ---- 12. vector env ----------------------------------------------------------------------------------------------------------------------
def test_vector_env_branch_for_the_whole_batch_and_for_a_group():
    from xroute_env_amd.envs.vector_env import XRouteVectorEnv
    regions = _mixed_regions()
    n = 24
    env = XRouteVectorEnv(regions, n_envs=n, device=DEV, max_route_count=1, groups=3, with_observation=False)
    env.reset()
    for s in range(2):
        env.step(env.random_actions(SEED + s))
    b = env.batch
    rng = np.random.default_rng(SEED + 12)
    before = _snap(b)
    parent = rng.integers(0, n, n)
    epoch = b.region_epoch
    assert env.branch(torch.as_tensor(parent.astype(np.int32), device=DEV)) is None
    assert b.region_epoch == epoch + 1
    _assert_gathered(b, before, parent, "whole batch")
    torch.cuda.synchronize()
    assert env.region.cpu().numpy().tolist() == before["region"][parent].tolist()
    assert env.legal.cpu().numpy().tobytes() == before["legal"][parent].tobytes()
    assert env.record.cpu().numpy().tobytes() == before["record"][parent].tobytes()
    env.step_async(env.random_actions(SEED + 5), 0)                # group 0 steps while group 1 branches
    lo, hi = b.group_bounds(1)
    mid = _snap(b)
    gp = rng.integers(0, hi - lo, hi - lo)
    env.branch(torch.as_tensor(gp.astype(np.int32), device=DEV), group=1)
    env.step_wait()
    torch.cuda.synchronize()
    after = _snap(b)
    for k in ROWS:
        assert after[k][lo:hi].tobytes() == mid[k][lo:hi][gp].tobytes(), k
        assert after[k][hi:].tobytes() == mid[k][hi:].tobytes(), k
    assert env.region[lo:hi].cpu().numpy().tolist() == mid["region"][lo:hi][gp].tolist()
    env.step(env.random_actions(SEED + 6))
    with pytest.raises(ValueError):
        env.branch(torch.zeros(n, dtype=torch.int32, device=DEV), group=3)
