"""Tree search (xr_batch_tree_search, XR-Tree v1) on the GPU: the device search against the spec's twin (tests/tree_twin.py) whose
returns come from RegionBatch.rollout, bit for bit; the best line against the oracle; lane counts, pool limits, region sizes, done envs,
purity, router variants, refusals, groups, the full-size batch, the vector env and whole episodes."""
import ctypes as C
import gc
import os

import numpy as np
import pytest
import torch

from tests import tree_twin
from xroute_env_amd import _lib
from xroute_env_amd.batch import RegionBatch
from xroute_env_amd.regions import generate_region

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x7EE5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAD = _lib.XR_ENV_BAD_ACTION
FULL = _lib.XR_TREE_POOL_FULL
FIELDS = ("paths", "returns", "visits", "value", "info", "best_order", "best_return")


@pytest.fixture(autouse=True)
def _release_cached_memory():
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _pack(sl=slice(None)):
    from xroute_env_amd.lefdef import load_region_pack
    return load_region_pack(os.path.join(GOLDEN, "ispd18_test1_regions.npz"))[sl]


def _mixed_regions():
    """Regions of different sizes (K <= 10), one with N % 8 != 0."""
    from tests.helpers import obs_set_regions
    extra = [generate_region(9100 + i, dims=d, k_range=(4, 10), pins=(3, 5), net_span=7)
             for i, d in enumerate([(16, 12, 5), (20, 14, 6), (13, 17, 4), (24, 20, 5)])]
    return obs_set_regions("mixed") + extra


def _snapshot(b):
    return {k: b.fetch(k).cpu().numpy().tobytes() for k in b._FETCH}


def _legal_rows(b, lo=0, hi=None):
    words = b.fetch("legal").cpu().numpy().view(np.uint64)
    bits = ((words[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).astype(bool)
    bits = bits.reshape(words.shape[0], -1)[lo:hi, :max(b.k_max, 1)]
    return [(np.flatnonzero(row) + 1).tolist() for row in bits]


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _advance(b, steps, history=None, start=0):
    for i in range(start, start + steps):
        act = b.random_actions(SEED + 1000 + i)
        b.step(act)
        if history is not None:
            for e, a in enumerate(act.cpu().numpy().tolist()):
                if a:
                    history[e].append(a)


def _twin(b, n_waves, n_par, seed, prior=None, node_cap=None, c_init=1.25, c_base=19652.0, group=None):
    """XR-Tree v1 in Python for the rows of `b` (or of one group): the returns of wave w are RegionBatch.rollout(n_par, seed_w, prefix =
    the wave's paths).  Returns a dict of numpy arrays shaped like tree_search(trace=True)'s and the RowTree objects."""
    K = max(b.k_max, 1)
    lo, hi = (0, b.n_envs) if group is None else b.group_bounds(group)
    legal = _legal_rows(b, lo, hi)
    rows = hi - lo
    cap = 1 + n_waves * n_par * K if node_cap is None else node_cap
    E = _lib.tree_exploration_table(c_init, c_base, n_waves * n_par)
    pri = None if prior is None else prior.cpu().numpy().tolist()

    def evaluate(w, paths):
        prefix = np.zeros((rows, n_par, K), np.int32)
        for r in range(rows):
            for j in range(n_par):
                prefix[r, j, :len(paths[r][j])] = paths[r][j]
        res = b.rollout(n_par, _lib.tree_seed(seed, w), prefix=torch.from_numpy(prefix).to(DEV), group=group)
        return res["ret"].cpu().numpy().tolist(), res["order"].cpu().numpy().tolist()

    results, paths, returns, trees = tree_twin.search(legal, n_waves, n_par, cap, E, evaluate, K, pri)
    out = dict(paths=np.array(paths, np.int32).reshape(rows, n_waves * n_par, K), returns=np.array(returns, np.float64).reshape(rows, n_waves * n_par),
               visits=np.array([r["visits"] for r in results], np.int32), value=np.array([r["value"] for r in results], np.float64),
               info=np.array([r["info"] for r in results], np.int32), best_order=np.array([r["best_order"] for r in results], np.int32),
               best_return=np.array([r["best_return"] for r in results], np.float64))
    return out, trees


def _assert_equal(dev, tw, what):
    for k in FIELDS:
        a, t = dev[k], tw[k]
        assert a.shape == t.shape and a.dtype == t.dtype, (what, k, a.shape, t.shape, a.dtype, t.dtype)
        if a.dtype == np.float64:
            a, t = a.view(np.uint64), t.view(np.uint64)
        assert np.array_equal(a, t), (what, k, np.argwhere(a != t)[:4].tolist())


def _search_both(b, n_waves, n_par, seed, what, **kw):
    before = _snapshot(b)
    dev = _np(b.tree_search(n_waves, n_par, seed, trace=True, **kw))
    assert _snapshot(b) == before, what
    tw, trees = _twin(b, n_waves, n_par, seed, **kw)
    _assert_equal(dev, tw, what)
    return dev, trees


def _random_prior(rows, K, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand((rows, K), generator=g, dtype=torch.float32)
    p[torch.rand((rows, K), generator=g) < 0.1] = 0.0
    p[0, 0], p[1 % rows, K - 1], p[2 % rows, 0] = float("nan"), -1.0, float("inf")          # entries that count as 0
    return p.to(DEV).contiguous()


# ---- 1. twin equivalence, bit for bit ----------------------------------------------------------------------------------------------
def test_the_device_search_equals_the_twin_bit_for_bit():
    regions = _mixed_regions()
    n = 24
    b = RegionBatch(regions, n_envs=n, device=DEV)
    b.reset()
    K = b.k_max
    assert K <= 10
    taken, depth, ties, terminal, differ = 0, 0, 0, 0, 0
    for at in (0, 2, 5):
        _advance(b, at - taken, start=taken)
        taken = at
        plain, t0 = _search_both(b, 4, 4, SEED + at, (at, "no prior"))
        prior = _random_prior(n, K, 77 + at)
        with_prior, t1 = _search_both(b, 4, 4, SEED + at, (at, "prior"), prior=prior)
        live = np.array([bool(t.legal) for t in t0])
        assert (plain["info"][live, 0] == 16).all() and not plain["info"][~live].any()
        for trees in (t0, t1):
            depth = max(depth, max(t.max_depth for t in trees))
            ties += sum(t.ties for t in trees)
            terminal += sum(t.terminal_visits for t in trees)
        differ += int(not np.array_equal(plain["paths"], with_prior["paths"]))
    # the inputs bite (the twin alone says so)
    assert depth >= 3 and ties > 0 and terminal > 0 and differ > 0, (depth, ties, terminal, differ)


# ---- 2. oracle ---------------------------------------------------------------------------------------------------------------------
def test_the_best_order_replayed_on_the_oracle_gives_the_bits_of_the_best_return():
    from oracle import xr_oracle as orc
    regions = _mixed_regions()
    n = 24
    b = RegionBatch(regions, n_envs=n, device=DEV)
    b.reset()
    history = [[] for _ in range(n)]
    _advance(b, 2, history)
    reg = b.fetch("region").cpu().numpy()
    legal = _legal_rows(b)
    res = _np(b.tree_search(4, 4, SEED, trace=True))
    checked = 0
    for e in range(n):
        if not legal[e]:
            assert res["best_return"][e] == -np.inf and not res["best_order"][e].any()
            continue
        assert res["best_return"][e] == res["returns"][e].max()
        first = int(np.argmax(res["returns"][e]))                                  # (the first maximum wins)
        nets = [int(v) for v in res["best_order"][e] if v > 0]
        assert sorted(nets) == legal[e], e
        p = [int(v) for v in res["paths"][e, first] if v > 0]
        assert nets[:len(p)] == p, (e, "the best order starts with its simulation's path")
        env = orc.OracleEnv(regions[int(reg[e])])
        env.reset()
        for a in history[e]:
            env.step(a)
        tot = 0.0
        for a in nets:
            ref = env.step(a)
            assert not ref["status"] & BAD
            tot = tot + orc.reward(*[int(v) for v in ref["delta"]])
        assert np.array([tot]).view(np.uint64)[0] == res["best_return"][e:e + 1].view(np.uint64)[0], (e, tot, res["best_return"][e])
        checked += 1
    assert checked >= 20


# ---- 3. lane counts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_waves,n_par", [(6, 1), (2, 16)])
def test_lane_counts(n_waves, n_par):
    regions = _mixed_regions()
    b = RegionBatch(regions, n_envs=24, device=DEV)
    b.reset()
    _advance(b, 1)
    dev, trees = _search_both(b, n_waves, n_par, SEED + n_par, (n_waves, n_par))
    live = np.array([bool(t.legal) for t in trees])
    assert (dev["info"][live, 0] == n_waves * n_par).all() and (dev["visits"].sum(axis=1)[live] == n_waves * n_par).all()
    if n_par == 16:
        assert any(len(t.legal) < 16 for t in trees if t.legal)                  # more lanes than legal nets
        assert dev["info"][:, 2].max() >= 2                                       # so the later lanes of wave 0 went a level down


# ---- 4. pool limits ----------------------------------------------------------------------------------------------------------------
def test_a_pool_of_one_node_leaves_the_root_unexpanded():
    regions = _mixed_regions()
    b = RegionBatch(regions, n_envs=24, device=DEV)
    b.reset()
    dev, trees = _search_both(b, 2, 4, SEED, "node_cap 1", node_cap=1)
    assert not dev["paths"].any() and not dev["visits"].any() and (dev["value"] == -np.inf).all()
    assert (dev["info"] == np.array([8, 1, 0, FULL], np.int32)).all()
    # every simulation is then a plain rollout: wave w is rollout(4, seed_w) without a prefix
    for w in range(2):
        assert np.array_equal(dev["returns"][:, 4 * w:4 * w + 4].view(np.uint64), b.rollout(4, _lib.tree_seed(SEED, w))["ret"].cpu().numpy().view(np.uint64))
    assert (dev["best_return"] == dev["returns"].max(axis=1)).all()


def test_a_pool_just_too_small_for_a_second_level():
    regions = [generate_region(9400, dims=(14, 12, 4), k_range=(5, 5), net_span=5)]
    b = RegionBatch(regions, n_envs=6, device=DEV)                               # one region in every slot: one block size
    b.reset()
    nl = b.fetch("nlegal").cpu().numpy()
    assert (nl == nl[0]).all() and nl[0] >= 3
    k = int(nl[0])
    cap = 1 + k + (k - 1) - 1                                                    # the root, its children, one node short of a child's block
    dev, _ = _search_both(b, 4, 4, SEED, "one short", node_cap=cap)
    assert (dev["info"][:, 1] == 1 + k).all() and (dev["info"][:, 2] == 1).all() and (dev["info"][:, 3] == FULL).all()
    assert (dev["visits"].sum(axis=1) == 16).all()
    dev, _ = _search_both(b, 4, 4, SEED, "exactly one block", node_cap=cap + 1)
    assert (dev["info"][:, 1] == 1 + k + k - 1).all() and (dev["info"][:, 2] <= 2).all() and (dev["info"][:, 3] == FULL).all()


# ---- 5. region sizes ---------------------------------------------------------------------------------------------------------------
def test_regions_with_one_and_two_nets():
    regions = [generate_region(9500 + i, dims=(10, 9, 4), k_range=(1 + i % 2, 1 + i % 2), net_span=5) for i in range(6)]
    b = RegionBatch(regions, device=DEV)
    b.reset()
    nl = b.fetch("nlegal").cpu().numpy()
    assert set(nl.tolist()) == {1, 2}
    dev, trees = _search_both(b, 4, 4, SEED, "1 and 2 nets")
    assert all(t.terminal_visits > 0 for t in trees)
    assert (dev["info"][:, 2] == nl).all() and (dev["info"][:, 3] == 0).all()
    assert (dev["info"][:, 1] == np.where(nl == 1, 2, 5)).all()                  # 1 + 1, and 1 + 2 + 1 + 1


def test_a_region_with_several_legal_words():
    from tests.helpers import OBS_MANY_NETS
    regions = [generate_region(9300, **OBS_MANY_NETS)]
    b = RegionBatch(regions, n_envs=1, device=DEV)
    assert b.legal_words >= 4
    b.reset()
    nets = _legal_rows(b)[0]
    assert len(nets) > 128 and max(nets) > 192                                   # more than 64 children, legal nets in the fourth word
    prior = torch.zeros((1, b.k_max), dtype=torch.float32, device=DEV)
    prior[0, nets[-1] - 1] = 5.0                                                 # the prior's favourite lives in the last word
    prior[0, nets[70] - 1] = 1.0
    cap = 1 + 5 * b.k_max                                                        # the root's block and one per simulation
    dev, _ = _search_both(b, 2, 2, SEED, "many nets", prior=prior, node_cap=cap)
    assert dev["info"][0].tolist()[0] == 4 and dev["info"][0, 3] == 0
    assert dev["paths"][0, 0, 0] == nets[0] and dev["paths"][0, 1, 0] == nets[-1]      # E[0] == 0: a tie; then E[1] > 0: the heaviest prior
    assert sorted(v for v in dev["best_order"][0].tolist() if v) == nets
    dev, _ = _search_both(b, 2, 2, SEED, "many nets, no prior")                 # the default pool: four blocks of ~200 nets, the fifth does not fit
    assert dev["info"][0, 3] == FULL
    assert dev["paths"][0, 0, 0] == nets[0] and dev["paths"][0, 1, 0] == nets[1]


# ---- 6. done envs ------------------------------------------------------------------------------------------------------------------
def test_done_envs_of_an_auto_reset_batch_hold_the_empty_result():
    regions = _mixed_regions()
    n = 24
    b = RegionBatch(regions, n_envs=n, device=DEV, auto_reset=True, max_route_count=1)
    b.reset()
    act = torch.empty(n, dtype=torch.int32, device=DEV)
    done_seen = live_seen = 0
    for step in range(10):
        nl = b.fetch("nlegal").cpu().numpy()
        res = _np(b.tree_search(2, 2, SEED + step, trace=True))
        done = nl == 0
        for k in ("visits", "info", "best_order", "paths"):
            assert not res[k][done].any(), (step, k)
        assert (res["value"][done] == -np.inf).all() and (res["best_return"][done] == -np.inf).all()
        assert (res["returns"][done].view(np.uint64) == 0).all()                   # +0.0
        assert (res["info"][~done, 0] == 4).all() and (res["visits"][~done].sum(axis=1) == 4).all()
        done_seen += int(done.sum()); live_seen += int((~done).sum())
        b.step(b.random_actions(SEED + step, act))
    assert done_seen > 0 and live_seen > 0


# ---- 7. purity ---------------------------------------------------------------------------------------------------------------------
def test_tree_search_leaves_every_fetchable_array_byte_identical():
    regions = _mixed_regions()
    b = RegionBatch(regions, n_envs=24, device=DEV, auto_reset=True, max_route_count=1)
    b.reset()
    act = torch.empty(24, dtype=torch.int32, device=DEV)
    for step in range(8):
        before = _snapshot(b)
        b.tree_search(2, 3, SEED + step)
        if step % 3 == 0:
            b.tree_search(1, 1, SEED, node_cap=2, trace=True)
            b.tree_search(3, 2, SEED, prior=_random_prior(24, b.k_max, step), c_init=0.5, c_base=100.0)
        after = _snapshot(b)
        for k in before:
            assert before[k] == after[k], (step, k)
        b.step(b.random_actions(SEED + step, act))


@pytest.mark.parametrize("mode", ["route", "inplace", "inplace_u8"])
def test_a_batch_that_searches_before_every_step_equals_its_twin_that_never_does(mode):
    regions = _mixed_regions()
    kw = dict(n_envs=24, device=DEV, auto_reset=True, max_route_count=1)
    a, t = RegionBatch(regions, **kw), RegionBatch(regions, **kw)
    a.reset(); t.reset()
    obs_a = obs_t = None
    if mode != "route":
        dt = torch.uint8 if mode == "inplace_u8" else torch.float32
        obs_a, obs_t = a.alloc_observation(dtype=dt).zero_(), t.alloc_observation(dtype=dt).zero_()
        a.observation(obs_a); t.observation(obs_t)
    act = torch.empty(24, dtype=torch.int32, device=DEV)
    for step in range(30):
        a.tree_search(2, 2, SEED + step)
        a.random_actions(SEED + step, act)
        a.step(act, obs_a, inplace=True) if obs_a is not None else a.step(act)
        t.step(act, obs_t, inplace=True) if obs_t is not None else t.step(act)
        for k in ("hash", "record", "owner", "legal", "region", "replay", "env_steps", "steps", "path", "path_len", "sweeps"):
            assert a.fetch(k).cpu().numpy().tobytes() == t.fetch(k).cpu().numpy().tobytes(), (step, k)
        if obs_a is not None:
            info = a.observe_info()
            assert info["form"] == 3 and info["inplace"], (step, info)          # the in-place path survived the search
            assert torch.equal(obs_a, obs_t), step


# ---- 8. router variants ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["auto", "sweep", "dial", "dial_r2", "v2_guides"])
def test_tree_search_under_every_router_variant(variant):
    if variant == "v2_guides":
        regions = _pack(slice(5, 200, 13))[:8]
        assert all(r.guide_off is not None and r.guide_off[-1] > 0 for r in regions)
        kw = dict(guide_cost=1000, guide_margin=1, maze_end_iter=3)
    else:
        regions = [generate_region(3000 + i, dims=(16, 14, 5), k_range=(3, 8)) for i in range(8)]
        kw = dict(router={"auto": 0, "sweep": 1, "dial": 2, "dial_r2": 3}[variant], dial_mult=0 if variant != "dial" else 5)
    b = RegionBatch(regions, device=DEV, **kw)
    b.reset()
    _search_both(b, 2, 3, SEED, (variant, 0))
    _advance(b, 2)
    dev, _ = _search_both(b, 2, 3, SEED + 1, (variant, 2))
    assert (dev["info"][:, 0] > 0).any()


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(force_scratch_field=True), dict(stream_per_region=True)])
def test_tree_search_refuses_the_scratch_forms_and_leaves_the_batch_untouched(kw):
    regions = [generate_region(3000 + i, dims=(12, 10, 4), k_range=(3, 6)) for i in range(4)]
    b = RegionBatch(regions, device=DEV, **kw)
    b.reset()
    b.step(b.random_actions(SEED))
    before = _snapshot(b)
    with pytest.raises(_lib.XRouteError) as ei:
        b.tree_search(2, 2, SEED)
    assert ei.value.code == _lib.XR_ERR_RANGE
    assert _snapshot(b) == before
    b.step(b.random_actions(SEED + 1))            # still usable


def test_tree_search_argument_errors_on_a_live_batch():
    regions = [generate_region(3000 + i, dims=(12, 10, 4), k_range=(3, 6)) for i in range(4)]
    b = RegionBatch(regions, device=DEV)
    b.reset()
    b.step(b.random_actions(SEED))
    K = b.k_max
    visits = torch.empty((4, K), dtype=torch.int32, device=DEV)
    value = torch.empty((4, K), dtype=torch.float64, device=DEV)
    info = torch.empty((4, 4), dtype=torch.int32, device=DEV)
    pv, pval, pi = (C.c_void_p(t.data_ptr()) for t in (visits, value, info))
    before = _snapshot(b)
    L = b.L
    nan, inf = float("nan"), float("inf")

    def call(group=-1, n_waves=2, n_par=2, node_cap=64, c_init=1.25, c_base=19652.0, visits=pv, value=pval, k_cap=K, info=pi):
        return L.xr_batch_tree_search(b._h, group, n_waves, n_par, 7, None, node_cap, c_init, c_base, visits, value, k_cap, info, None, None, None, None,
                                      None)

    INV, RNG = _lib.XR_ERR_INVALID, _lib.XR_ERR_RANGE
    for kw, code, word in ((dict(visits=None), INV, b"null"), (dict(value=None), INV, b"null"), (dict(info=None), INV, b"null"),
                           (dict(group=1), INV, b"group"), (dict(group=-2), INV, b"group"), (dict(n_waves=0), INV, b"n_waves"),
                           (dict(n_par=0), INV, b"n_par"), (dict(c_init=nan), INV, b"c_init"), (dict(c_init=inf), INV, b"c_init"),
                           (dict(c_base=0.0), INV, b"c_base"), (dict(c_base=-2.0), INV, b"c_base"), (dict(c_base=nan), INV, b"c_base"),
                           (dict(n_par=_lib.XR_ROLLOUT_MAX + 1), RNG, b"n_par"), (dict(n_waves=17, n_par=4096), RNG, b"simulations"),
                           (dict(node_cap=0), RNG, b"node_cap"), (dict(node_cap=-5), RNG, b"node_cap"), (dict(k_cap=K - 1), RNG, b"k_cap")):
        assert call(**kw) == code, kw
        msg = L.xr_last_error()
        assert b"xr_batch_tree_search" in msg and word in msg, (kw, msg)
    assert _snapshot(b) == before
    for bad in (dict(n_waves=0), dict(n_par=0), dict(c_base=0.0), dict(node_cap=0), dict(prior=torch.zeros((4, K), dtype=torch.float64, device=DEV))):
        with pytest.raises(ValueError):
            b.tree_search(**dict(dict(n_waves=2, n_par=2), **bad))
    # a valid raw call with the optional outputs null, and a wider k_cap: the columns past k_max hold 0 / -inf
    assert call() == 0
    wide_v = torch.full((4, K + 3), 77, dtype=torch.int32, device=DEV)
    wide_val = torch.zeros((4, K + 3), dtype=torch.float64, device=DEV)
    assert call(visits=C.c_void_p(wide_v.data_ptr()), value=C.c_void_p(wide_val.data_ptr()), k_cap=K + 3) == 0
    res = b.tree_search(2, 2, 7, node_cap=64)
    assert torch.equal(res["visits"], visits) and torch.equal(res["info"], info) and torch.equal(res["value"], value)
    assert torch.equal(wide_v[:, :K], visits) and not wide_v[:, K:].any() and bool((wide_val[:, K:] == -inf).all())
    assert _snapshot(b) == before
    b.step(b.random_actions(SEED + 1))            # still usable


# ---- 10. groups --------------------------------------------------------------------------------------------------------------------
def test_groups_search_on_their_own_streams_between_steps_of_other_groups():
    regions = [generate_region(3000 + i, dims=(16, 14, 5), k_range=(3, 8)) for i in range(8)] + _mixed_regions()[:6]
    n = 40
    kw = dict(n_envs=n, device=DEV, auto_reset=True, max_route_count=1)
    a, t = RegionBatch(regions, **kw), RegionBatch(regions, **kw)
    a.set_groups(4)
    a.reset(); t.reset()
    K = a.k_max
    prior = _random_prior(n, K, 5)
    torch.cuda.synchronize()
    cur = torch.cuda.current_stream()
    streams = [torch.cuda.Stream() for _ in range(4)]
    cadence = [1, 2, 3, 2]
    rounds = 3
    results = {g: [] for g in range(4)}
    for s in streams:
        s.wait_stream(cur)
    for r in range(rounds):
        for k in range(max(cadence)):
            for g in range(4):
                if k >= cadence[g]:
                    continue
                s = streams[g]
                lo, hi = a.group_bounds(g)
                with torch.cuda.stream(s):
                    results[g].append(a.tree_search(2, 3, SEED, prior=prior[lo:hi], group=g, stream=s, trace=True))
                    act = a.random_actions_group(g, SEED, stream=s)
                    a.step_group(g, act, stream=s)
    for s in streams:
        cur.wait_stream(s)
    torch.cuda.synchronize()
    twin = []
    act = torch.empty(n, dtype=torch.int32, device=DEV)
    for i in range(rounds * max(cadence)):
        twin.append(_np(t.tree_search(2, 3, SEED, prior=prior, trace=True)))
        t.step(t.random_actions(SEED, act))
    for g in range(4):
        lo, hi = a.group_bounds(g)
        assert len(results[g]) == rounds * cadence[g]
        for i, res in enumerate(results[g]):
            _assert_equal(_np(res), {k: v[lo:hi] for k, v in twin[i].items()}, (g, i))


# ---- 11. full size -----------------------------------------------------------------------------------------------------------------
def test_tree_search_at_4096_ispd18_slots():
    b = RegionBatch(_pack(), n_envs=4096, device=DEV, auto_reset=False)
    b.reset()
    _advance(b, 3)
    nl = b.fetch("nlegal").cpu().numpy()
    res = b.tree_search(2, 2, SEED, node_cap=1 + 5 * b.k_max, trace=True)          # (the root's block and one per simulation: never full)
    ro = b.rollout(2, _lib.tree_seed(SEED, 0), prefix=res["paths"][:, :2].contiguous())
    assert torch.equal(res["returns"][:, 0].view(torch.int64), ro["ret"][:, 0].view(torch.int64))
    assert torch.equal(res["returns"][:, 1].view(torch.int64), ro["ret"][:, 1].view(torch.int64))
    res = _np(res)
    live = nl > 0
    assert live.sum() > 2048
    info = res["info"]
    assert (info[live, 0] == 4).all() and not info[~live].any()
    assert (info[live, 1] >= 1 + nl[live]).all() and (info[live, 1] <= 1 + 5 * b.k_max).all()
    assert (info[live, 2] >= 1).all() and (info[live, 2] <= nl[live]).all() and (info[:, 3] == 0).all()
    assert (res["visits"].sum(axis=1)[live] == 4).all()
    assert (res["best_return"][live] == res["returns"][live].max(axis=1)).all()
    legal = _legal_rows(b)
    firsts = np.array([l[0] if l else 0 for l in legal], np.int32)
    assert np.array_equal(res["paths"][:, 0, 0], firsts)                          # wave 0, lane 0: every score is 0, the lowest net


# ---- 12. vector env and episodes ---------------------------------------------------------------------------------------------------
def test_vector_env_tree_actions_and_an_episode_driven_by_them():
    from xroute_env_amd.envs.vector_env import XRouteVectorEnv
    regions = _mixed_regions()
    env = XRouteVectorEnv(regions, n_envs=24, device=DEV, max_route_count=1)
    env.reset()
    k_most = max(r.n_nets for r in regions)
    finished = np.zeros(24, bool)
    for step in range(k_most + 2):
        res = _np(env.tree_search(3, 4, SEED + step))
        act = env.tree_actions(3, 4, SEED + step).cpu().numpy()
        nl = env.batch.fetch("nlegal").cpu().numpy()
        assert np.array_equal(act == 0, nl == 0)
        for e in range(24):                                                       # most visited, then the higher value, then the lower net
            if nl[e]:
                key = [(-int(v), -float(val), i + 1) for i, (v, val) in enumerate(zip(res["visits"][e], res["value"][e])) if v > 0]
                assert act[e] == min(key)[2], (step, e)
        _, _, done, info = env.step(torch.from_numpy(act).to(DEV))
        rec = env.batch.records()
        assert not (rec["status"][nl > 0] & BAD).any(), step
        finished |= done.cpu().numpy().astype(bool)
    assert finished.all()


def test_vector_env_group_tree_actions_equal_the_whole_batch_rows():
    from xroute_env_amd.envs.vector_env import XRouteVectorEnv
    regions = _mixed_regions()
    env = XRouteVectorEnv(regions, n_envs=24, device=DEV, max_route_count=1, groups=3, with_observation=False)
    env.reset()
    whole = env.tree_actions(2, 3, SEED).cpu().numpy()
    for g in range(3):
        lo, hi = env.batch.group_bounds(g)
        act = env.tree_actions(2, 3, SEED, group=g)
        env.step_wait(g)
        assert np.array_equal(act.cpu().numpy(), whole[lo:hi])
        env.step_async(act, g)
    env.step_wait()
    torch.cuda.synchronize()


def test_tree_episodes_return_permutations_of_every_regions_nets():
    from oracle import xr_oracle as orc
    from xroute_env_amd.envs.tree import lookahead_prior, tree_episodes
    regions = _mixed_regions()[:8]
    stats = {}
    for prior in (None, lambda batch: lookahead_prior(batch, 2.0)):
        out = tree_episodes(regions, 2, 4, seed=SEED, device=DEV, prior=prior, stats=stats)
        assert len(out) == len(regions) and stats["routed_nets"] > 0
        for r, o in zip(regions, out):
            env = orc.OracleEnv(r)
            env.reset()
            nets = sorted(int(v) for v in env.legal())
            assert sorted(o["order"]) == nets and sorted(o["best_order"]) == nets          # permutations of the region's nets
            tot = 0.0
            for a in o["order"]:
                ref = env.step(a)
                assert not ref["status"] & BAD
                tot = tot + orc.reward(*[int(v) for v in ref["delta"]])
            assert env.nlegal() == 0 and tot == o["ret"]
            assert o["best_ret"] > -np.inf and o["simulations"] == 8 * len(o["order"])
