"""Kept trees (xr_batch_tree_search_keep, "XR-Tree v1, kept") on the GPU: the device search against the spec's twin
(tests/tree_keep_twin.py) whose returns come from RegionBatch.rollout, bit for bit — fresh calls against the plain search, whole episodes
of search -> step the most visited net -> continue, played == 0, every rebuild case, an exactly filled pool, purity, groups, refusals.

Shapes: 3-6 envs of generate_region regions with 1, 2, 5 and 65-70 nets (the last: child blocks above one wavefront), n_par in {1, 3},
n_waves in {1, 4}.  Test conditions of the episodes (the twin alone says whether the inputs meet them): every row that is live before
and after a step and whose played net hung below an expanded root shows XR_TREE_KEPT in the next search; every search but the first
that has a live row has at least one such row; at least one row has 3 nets or more."""
import gc

import numpy as np
import pytest
import torch

from tests import tree_keep_twin as kt
from xroute_env_amd import _lib
from xroute_env_amd.batch import RegionBatch
from xroute_env_amd.envs.vector_env import XRouteVectorEnv
from xroute_env_amd.regions import generate_region

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x4EE9
KEPT, FULL = _lib.XR_TREE_KEPT, _lib.XR_TREE_POOL_FULL
FIELDS = ("paths", "returns", "visits", "value", "info", "best_order", "best_return", "kept")
PLAIN = FIELDS[:-1]
_TABLE = {}


@pytest.fixture(autouse=True)
def _release_cached_memory():
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _small_regions():
    """Five regions with 1, 2, 5, 5 and 3 nets."""
    return [generate_region(9600 + i, dims=(12, 10, 4), k_range=(k, k), net_span=5) for i, k in enumerate((1, 2, 5, 5, 3))]


def _wide_regions():
    """Three regions, one with 65-70 nets: its root's block is wider than one wavefront."""
    return [generate_region(9650, dims=(23, 15, 5), k_range=(65, 70), net_span=6, pins=(2, 2), aps=(1, 1)),
            generate_region(9651, dims=(12, 10, 4), k_range=(5, 5), net_span=5), generate_region(9652, dims=(12, 10, 4), k_range=(2, 2), net_span=5)]


def _E(c_init=1.25, c_base=19652.0):
    if (c_init, c_base) not in _TABLE:
        _TABLE[(c_init, c_base)] = _lib.tree_exploration_table(c_init, c_base, kt.MAX_SIMS)
    return _TABLE[(c_init, c_base)]


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _snapshot(b):
    return {k: b.fetch(k).cpu().numpy().tobytes() for k in b._FETCH}


def _states(b, lo=0, hi=None):
    K = max(b.k_max, 1)
    words = b.fetch("legal").cpu().numpy().view(np.uint64)
    bits = ((words[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).astype(bool).reshape(words.shape[0], -1)[:, :K]
    steps, region, replay, reward = (b.fetch(k).cpu().numpy() for k in ("env_steps", "region", "replay", "reward"))
    return [kt.State(steps[e], region[e], replay[e], (np.flatnonzero(bits[e]) + 1).tolist(), reward[e]) for e in range(lo, b.n_envs if hi is None else hi)]


def _weights(rows, k, seed):
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 1000, size=(rows, k), dtype=np.int64)
    w[rng.random((rows, k)) < 0.15] = 0
    return torch.from_numpy(w.astype(np.int32)).to(DEV).contiguous()


class Twin:
    """The kept-tree pool of one caller of `b` (the whole batch, or a group) in Python: wave w's returns are RegionBatch.rollout(n_par,
    seed_w, prefix = the wave's paths) of `b`, random or weighted."""

    def __init__(self, b, group=None):
        self.b, self.group, self.pool = b, group, kt.KeptPool()
        self.lo, self.hi = (0, b.n_envs) if group is None else b.group_bounds(group)

    def search(self, played, n_waves, n_par, seed, node_cap, prior=None, sim_weights=None):
        b, rows, K = self.b, self.hi - self.lo, max(self.b.k_max, 1)

        def evaluate(w, paths):
            prefix = np.zeros((rows, n_par, K), np.int32)
            for r in range(rows):
                for j in range(n_par):
                    prefix[r, j, :len(paths[r][j])] = paths[r][j]
            kw = dict(policy="weighted", weights=sim_weights) if sim_weights is not None else {}
            res = b.rollout(n_par, _lib.tree_seed(seed, w), prefix=torch.from_numpy(prefix).to(DEV), group=self.group, **kw)
            return res["ret"].cpu().numpy().tolist(), res["order"].cpu().numpy().tolist()

        pl = None if played is None else played.cpu().numpy().tolist()
        pri = None if prior is None else prior.cpu().numpy().tolist()
        results, paths, returns, trees = self.pool.search(_states(b, self.lo, self.hi), pl, n_waves, n_par, node_cap, _E(), evaluate, K, pri, lo=self.lo)
        S = n_waves * n_par
        out = dict(paths=np.array(paths, np.int32).reshape(rows, S, K), returns=np.array(returns, np.float64).reshape(rows, S),
                   visits=np.array([r["visits"] for r in results], np.int32), value=np.array([r["value"] for r in results], np.float64),
                   info=np.array([r["info"] for r in results], np.int32), best_order=np.array([r["best_order"] for r in results], np.int32),
                   best_return=np.array([r["best_return"] for r in results], np.float64), kept=np.array([r["kept"] for r in results], np.int32))
        return out, trees


def _assert_equal(dev, tw, what, fields=FIELDS):
    for k in fields:
        a, t = dev[k], tw[k]
        assert a.shape == t.shape and a.dtype == t.dtype, (what, k, a.shape, t.shape, a.dtype, t.dtype)
        if a.dtype == np.float64:
            a, t = a.view(np.uint64), t.view(np.uint64)
        assert np.array_equal(a, t), (what, k, np.argwhere(a != t)[:4].tolist())


def _both(b, twin, played, n_waves, n_par, seed, node_cap, what, **kw):
    """One kept call on the device and in the twin: equal in every output; the batch untouched."""
    before = _snapshot(b)
    dev = _np(b.tree_search(n_waves, n_par, seed, node_cap=node_cap, trace=True, keep=True, played=played, group=twin.group, **kw))
    assert _snapshot(b) == before, what
    tw, trees = twin.search(played, n_waves, n_par, seed, node_cap, **kw)
    _assert_equal(dev, tw, what)
    return dev, trees


def _act(res):
    return XRouteVectorEnv._most_visited({k: torch.from_numpy(v).to(DEV) for k, v in res.items() if k in ("visits", "value", "best_order")})


# ---- 1. a fresh kept call is the plain search --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_waves,n_par", [(1, 1), (4, 3)])
@pytest.mark.parametrize("regions", ["small", "wide"])
def test_played_none_equals_the_plain_search_and_leaves_its_next_call_unchanged(regions, n_waves, n_par):
    regs = _small_regions() if regions == "small" else _wide_regions()
    b = RegionBatch(regs, device=DEV)
    b.reset()
    K = b.k_max
    cap = 1 + (n_waves * n_par + 1) * K
    for w in (None, _weights(b.n_envs, K, 3)):
        kw = dict(node_cap=cap, trace=True, sim_weights=w)
        plain = _np(b.tree_search(n_waves, n_par, SEED, **kw))
        kept = _np(b.tree_search(n_waves, n_par, SEED, keep=True, **kw))
        _assert_equal(kept, plain, (regions, "keep vs plain", w is not None), PLAIN)
        assert not kept["kept"].any() and not (kept["info"][:, 3] & KEPT).any()
        _assert_equal(_np(b.tree_search(n_waves, n_par, SEED, **kw)), plain, (regions, "plain again"), PLAIN)
        b.tree_search(2, 2, SEED + 1, node_cap=cap)                                  # the plain pool holds another search now:
        again = _np(b.tree_search(n_waves, n_par, SEED, keep=True, played=torch.zeros(b.n_envs, dtype=torch.int32, device=DEV), **kw))
        assert (again["kept"][:, 0] == n_waves * n_par).all()                       # the kept trees are still there
    if regions == "wide":
        assert b.fetch("nlegal").cpu().numpy()[0] > 64


# ---- 2. whole episodes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_an_episode_of_search_step_continue_equals_the_twin_at_every_ply(weighted):
    b = RegionBatch(_small_regions(), device=DEV, auto_reset=False)
    b.reset()
    K, n = b.k_max, b.n_envs
    twin = Twin(b)
    w = _weights(n, K, 11) if weighted else None
    cap = 1 + 4 * 4 * 3 * K
    played, kept_searches, deep = None, 0, 0
    for ply in range(K + 1):
        live = np.array([bool(s.legal) for s in _states(b)])
        if not live.any():
            break
        old = [r.tree for r in twin.pool.rows] if twin.pool.rows else None
        dev, trees = _both(b, twin, played, 4, 3, SEED + ply, cap, ("episode", weighted, ply), sim_weights=w)
        if played is not None:
            pl = played.cpu().numpy()
            must = np.array([live[e] and pl[e] > 0 and old[e] is not None and bool(old[e].nodes) and old[e].nodes[0].first >= 0 for e in range(n)])
            assert ((dev["info"][must, 3] & KEPT) != 0).all(), ply
            assert must.any(), ("no row shows a kept tree", ply)
            assert (dev["kept"][must, 0] > 0).any()
            kept_searches += 1
            deep = max(deep, int(dev["kept"][:, 1].max()))
            # the carried visits are in the root's counts
            grown = must & (dev["kept"][:, 1] > 1)          # (a carried root that had left its first visit behind: that one stopped at it)
            assert (dev["visits"].sum(axis=1)[grown] == dev["kept"][grown, 0] - 1 + 12).all(), ply
        else:
            assert sum(len(s.legal) >= 3 for s in _states(b)) >= 1
        act = _act(dev)
        b.step(act)
        played = act
    assert kept_searches >= 4 and deep > 3 and not (b.fetch("nlegal") > 0).any()


def test_three_plies_of_a_region_whose_blocks_are_wider_than_a_wavefront():
    b = RegionBatch(_wide_regions(), device=DEV, auto_reset=False)
    b.reset()
    K = b.k_max
    assert b.fetch("nlegal").cpu().numpy()[0] > 64 and b.legal_words >= 2
    twin = Twin(b)
    cap = 1 + 40 * K                                                             # the root's block and one per simulation of the three plies
    prior = torch.rand((b.n_envs, K), generator=torch.Generator().manual_seed(5), dtype=torch.float32).to(DEV).contiguous()
    played = None
    for ply in range(3):
        dev, trees = _both(b, twin, played, 4, 3 if ply else 1, SEED + ply, cap, ("wide", ply), prior=prior)
        if ply:
            assert dev["info"][0, 3] == KEPT and dev["kept"][0, 1] > 64          # a block above 64 nodes was copied
        act = _act(dev)
        b.step(act)
        played = act


# ---- 3. the env has not moved ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_par", [1, 3])
def test_played_zero_adds_simulations_to_the_same_root(n_par):
    b = RegionBatch(_small_regions(), device=DEV, auto_reset=False)
    b.reset()
    twin = Twin(b)
    cap = 1 + 8 * n_par * b.k_max
    zero = torch.zeros(b.n_envs, dtype=torch.int32, device=DEV)
    first, _ = _both(b, twin, None, 2, n_par, SEED, cap, "first half")
    second, trees = _both(b, twin, zero, 2, n_par, SEED + 1, cap, "second half")
    assert (second["info"][:, 3] == KEPT).all() and (second["kept"][:, 0] == 2 * n_par).all()
    assert np.array_equal(second["kept"][:, 1], first["info"][:, 1])
    assert (second["visits"].sum(axis=1) == 4 * n_par).all() and all(t.nodes[0].N == 4 * n_par for t in trees)
    assert (second["info"][:, 0] == 2 * n_par).all()
    # n_par, n_waves, the knobs and the seed may differ: still kept
    third = _np(b.tree_search(1, 2, SEED + 2, node_cap=cap, keep=True, played=zero, c_init=0.5, c_base=100.0))
    assert (third["info"][:, 3] & KEPT).all() and (third["kept"][:, 0] == 4 * n_par).all()


# ---- 4. rebuilds -------------------------------------------------------------------------------------------------------------------
def _fresh_rows(b, dev, rows, n_waves, n_par, seed, cap, what):
    """The rows `rows` of a kept call equal a fresh search of the state the batch is in; the other live rows are kept."""
    plain = _np(b.tree_search(n_waves, n_par, seed, node_cap=cap, trace=True))
    rows = np.array(rows)
    _assert_equal({k: dev[k][rows] for k in PLAIN}, {k: plain[k][rows] for k in PLAIN}, what, PLAIN)
    assert not dev["kept"][rows].any(), what
    others = np.setdiff1d(np.flatnonzero(b.fetch("nlegal").cpu().numpy() > 0), rows)
    assert len(others) and (dev["info"][others, 3] & KEPT).all(), what


def _started(groups=None, **kw):
    b = RegionBatch(_small_regions()[2:] + _small_regions()[2:4], device=DEV, **kw)          # 5, 5, 3, 5, 5 nets
    if groups:
        b.set_groups(groups)
    b.reset()
    twin = Twin(b)
    cap = 1 + 4 * 2 * 3 * b.k_max
    dev, _ = _both(b, twin, None, 2, 3, SEED, cap, "start")
    return b, twin, cap, _act(dev)


def test_a_wrong_net_and_a_negative_entry_rebuild_their_rows():
    b, twin, cap, act = _started()
    b.step(act)
    played = act.clone()
    legal = _states(b)[1].legal
    played[1] = legal[0]                                        # a net that was legal and was not the one played
    played[3] = -7
    dev, _ = _both(b, twin, played, 2, 3, SEED + 1, cap, "wrong net")
    _fresh_rows(b, dev, [1, 3], 2, 3, SEED + 1, cap, "wrong net")


def test_envs_not_stepped_and_stepped_twice_rebuild_their_rows():
    b, twin, cap, act = _started(groups=[0, 2, 3, 5])
    b.step_group(0, act[0:2].contiguous())                      # group 0: one step; group 1: none; group 2: two
    b.step_group(2, act[3:5].contiguous())
    b.step_group(2, b.random_actions_group(2, SEED))
    torch.cuda.synchronize()
    dev, _ = _both(b, twin, act, 2, 3, SEED + 1, cap, "no step, two steps")
    _fresh_rows(b, dev, [2, 3, 4], 2, 3, SEED + 1, cap, "no step, two steps")
    # told the truth (played 0) the row that has not moved is kept whole
    played = torch.tensor([-1, -1, 0, -1, -1], dtype=torch.int32, device=DEV)
    dev, _ = _both(b, twin, played, 2, 3, SEED + 2, cap, "no step, played 0")
    assert dev["info"][2, 3] == KEPT and dev["kept"][2, 0] == 6 and not dev["kept"][[0, 1, 3, 4]].any()


def test_an_auto_reset_between_the_calls_rebuilds_the_row():
    regs = _small_regions()
    b = RegionBatch([regs[0], regs[2], regs[3]], device=DEV, auto_reset=True, max_route_count=1)          # 1, 5, 5 nets
    b.reset()
    twin = Twin(b)
    cap = 1 + 4 * 6 * b.k_max
    played = None
    seen = []
    for ply in range(3):
        dev, _ = _both(b, twin, played, 2, 3, SEED + ply, cap, ("auto reset", ply))
        seen.append((dev["info"][0].tolist(), dev["kept"][0].tolist()))
        act = _act(dev)
        b.step(act)
        played = act
    # row 0: a fresh tree, then a done row (its only net was played), then — the env has reset under it — a fresh tree again
    assert seen[0][0][0] == 6 and seen[1] == ([0, 0, 0, 0], [0, 0]) and seen[2][0][0] == 6 and seen[2][0][3] == 0 and seen[2][1] == [0, 0]
    assert (dev["info"][1:, 3] == KEPT).all()


def test_a_branch_from_a_slot_of_another_region_rebuilds_the_row():
    b, twin, cap, act = _started()
    b.step(act)
    b.branch(torch.tensor([0, 1, 1, 3, 4], dtype=torch.int32, device=DEV))          # slot 2 (3 nets) takes slot 1's state (another region)
    dev, _ = _both(b, twin, act, 2, 3, SEED + 1, cap, "branch")
    _fresh_rows(b, dev, [2], 2, 3, SEED + 1, cap, "branch")


def test_a_changed_node_cap_rebuilds_every_row():
    b, twin, cap, act = _started()
    b.step(act)
    dev, _ = _both(b, twin, act, 2, 3, SEED + 1, cap + 1, "node_cap + 1")
    assert not dev["kept"].any() and not (dev["info"][:, 3] & KEPT).any()
    _assert_equal(dev, _np(b.tree_search(2, 3, SEED + 1, node_cap=cap + 1, trace=True)), "node_cap + 1", PLAIN)
    act = _act(dev)
    b.step(act)
    dev, _ = _both(b, twin, act, 2, 3, SEED + 2, cap + 1, "the same shape again")
    assert (dev["info"][:, 3] & KEPT).all()


# ---- 5. a pool filled to the last node ---------------------------------------------------------------------------------------------
def test_a_pool_the_continued_tree_fills_exactly_and_one_more_simulation_overflows():
    def run(cap, waves2):
        b = RegionBatch(_small_regions()[2:4], device=DEV, auto_reset=False)          # two rows of 5 nets; a batch of its own per run: the same state
        b.reset()
        twin = Twin(b)
        dev, _ = _both(b, twin, None, 3, 1, SEED, cap, ("first", cap))
        act = _act(dev)
        b.step(act)
        return _both(b, twin, act, waves2, 1, SEED + 1, cap, ("second", cap, waves2))[0]
    roomy = run(1000, 6)
    cap = int(roomy["info"][0, 1])
    assert roomy["kept"][0, 1] < cap and roomy["info"][0, 3] == KEPT
    exact = run(cap, 6)
    assert exact["info"][0].tolist() == [6, cap, roomy["info"][0, 2], KEPT]          # full to the last node, and nobody has noticed
    _assert_equal({k: v[:1] for k, v in exact.items()}, {k: v[:1] for k, v in roomy.items()}, "exact")
    over = run(cap, 7)
    assert over["info"][0, :2].tolist() == [7, cap] and over["info"][0, 3] == KEPT | FULL


# ---- 6. purity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])
def test_kept_searches_leave_the_batch_and_its_in_place_observation_alone(dtype):
    regs = _small_regions()
    kw = dict(n_envs=6, device=DEV, auto_reset=True, max_route_count=1)
    a, t = RegionBatch(regs, **kw), RegionBatch(regs, **kw)
    a.reset(); t.reset()
    obs_a, obs_t = a.alloc_observation(dtype=dtype).zero_(), t.alloc_observation(dtype=dtype).zero_()
    a.observation(obs_a); t.observation(obs_t)
    played = None
    for step in range(6):
        before = _snapshot(a)
        res = a.tree_search(2, 3, SEED + step, node_cap=200, keep=True, played=played)
        assert step == 0 or bool((res["info"][:, 3] & KEPT).any())
        a.tree_search(1, 1, SEED, node_cap=200, keep=True, played=torch.zeros(6, dtype=torch.int32, device=DEV))
        after = _snapshot(a)
        for k in before:
            assert before[k] == after[k], (step, k)
        act = XRouteVectorEnv._most_visited(res)
        a.step(act, obs_a, inplace=True)
        t.step(act, obs_t, inplace=True)
        info = a.observe_info()
        assert info["form"] == 3 and info["inplace"], (step, info)          # the in-place path survived the searches
        assert torch.equal(obs_a, obs_t), step
        for k in ("hash", "record", "owner", "legal", "env_steps"):
            assert a.fetch(k).cpu().numpy().tobytes() == t.fetch(k).cpu().numpy().tobytes(), (step, k)
        played = act


# ---- 7. groups ---------------------------------------------------------------------------------------------------------------------
def test_a_groups_kept_tree_and_the_whole_batchs_are_independent():
    b, whole, cap, act = _started(groups=[0, 2, 5])
    g1 = Twin(b, group=1)
    dev_g, _ = _both(b, g1, None, 1, 3, SEED + 50, cap, "group 1, start")
    b.step(act)
    dev, _ = _both(b, whole, act, 2, 3, SEED + 1, cap, "whole batch, continued")
    dev_g, _ = _both(b, g1, act[2:5].contiguous(), 2, 3, SEED + 51, cap, "group 1, continued")
    live = b.fetch("nlegal").cpu().numpy() > 0
    assert (dev["info"][live, 3] & KEPT).all() and (dev_g["info"][live[2:5], 3] & KEPT).all()
    assert (dev["kept"][2:5, 0] != dev_g["kept"][:, 0]).any()          # two different trees of the same rows
    assert not b.tree_search(1, 1, SEED, node_cap=cap, keep=True, played=act[0:2].contiguous(), group=0)["kept"].any()          # group 0 had none


def test_two_groups_on_two_streams_equal_their_lock_step_twins():
    regs = _small_regions()[2:] + _small_regions()[2:4]
    kw = dict(device=DEV, auto_reset=False)
    a, t = RegionBatch(regs, **kw), RegionBatch(regs, **kw)
    for x in (a, t):
        x.set_groups([0, 2, 5])
        x.reset()
    cap = 1 + 4 * 6 * a.k_max
    torch.cuda.synchronize()
    cur = torch.cuda.current_stream()
    streams = [torch.cuda.Stream() for _ in range(2)]
    results = {0: [], 1: []}
    plies = 3
    for g, s in enumerate(streams):
        s.wait_stream(cur)
        with torch.cuda.stream(s):
            played = None
            for ply in range(plies):
                res = a.tree_search(2, 3, SEED + 7 * g + ply, node_cap=cap, trace=True, keep=True, played=played, group=g, stream=s)
                act = XRouteVectorEnv._most_visited(res)
                a.step_group(g, act, stream=s)
                results[g].append(res)
                played = act
    for s in streams:
        cur.wait_stream(s)
    torch.cuda.synchronize()
    for g in range(2):
        twin, played = Twin(t, group=g), None
        for ply in range(plies):
            tw, _ = twin.search(played, 2, 3, SEED + 7 * g + ply, cap)
            _assert_equal(_np(results[g][ply]), tw, (g, ply))
            played = _act(tw)
            t.step_group(g, played)
        assert (tw["info"][:, 3] & KEPT).any()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(force_scratch_field=True), dict(stream_per_region=True)])
def test_the_kept_search_refuses_the_scratch_forms_by_name(kw):
    regions = [generate_region(3000 + i, dims=(12, 10, 4), k_range=(3, 6)) for i in range(4)]
    b = RegionBatch(regions, device=DEV, **kw)
    b.reset()
    before = _snapshot(b)
    with pytest.raises(_lib.XRouteError) as ei:
        b.tree_search(2, 2, SEED, keep=True)
    assert ei.value.code == _lib.XR_ERR_RANGE and "xr_batch_tree_search_keep" in str(ei.value)
    assert _snapshot(b) == before
    b.step(b.random_actions(SEED))            # still usable
