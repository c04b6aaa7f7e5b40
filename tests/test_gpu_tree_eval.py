"""Evaluated tree search (xr_batch_tree_open / _leaves / _backup, "XR-Tree v2, evaluated") on the GPU: the device session against the
spec's twin (tests/tree_eval_twin.py) under a synthetic, state-dependent evaluator, bit for bit after every wave; the anchor to the
rollout search (values that complete each line to a rollout's return reproduce tree_search); the leaves against peek; wide blocks, one
net, done envs, full pools, max_sims, re-opening; purity and coexistence with the plain and the kept search; env groups on their own
streams; the critic and actor-critic evaluators on the ispd18 pack; whole episodes."""
import gc
import os

import numpy as np
import pytest
import torch

from tests import tree_eval_twin as et
from xroute_env_amd import _lib
from xroute_env_amd.batch import RegionBatch
from xroute_env_amd.regions import generate_region

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x7EE6
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAD = _lib.XR_ENV_BAD_ACTION
FULL = _lib.XR_TREE_POOL_FULL
TERMINAL, FRESH, NONE = _lib.XR_TREE_LEAF_TERMINAL, _lib.XR_TREE_LEAF_FRESH, _lib.XR_TREE_LEAF_NONE
RESULT = ("visits", "value", "info", "best_order", "best_return", "returns")


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
    """tests/test_gpu_tree.py's set: regions of different sizes (K <= 10), one with N % 8 != 0."""
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


def _advance(b, steps, start=0):
    for i in range(start, start + steps):
        b.step(b.random_actions(SEED + 1000 + i))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, t, what):
    assert a.shape == t.shape and a.dtype == t.dtype, (what, a.shape, t.shape, a.dtype, t.dtype)
    assert np.array_equal(_bits(a), _bits(t)), (what, np.argwhere(_bits(a) != _bits(t))[:4].tolist())


def _random_prior(rows, K, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand((rows, K), generator=g, dtype=torch.float32)
    p[torch.rand((rows, K), generator=g) < 0.1] = 0.0
    p[0, 0], p[1 % rows, K - 1], p[2 % rows, 0] = float("nan"), -1.0, float("inf")          # entries that count as 0
    return p.to(DEV).contiguous()


def _synthetic(leaves, K, with_prior):
    """An evaluator that depends on the leaf's STATE alone: a hash of the packed row's bytes -> a value that is no dyadic number (every
    addition rounds), now and then NaN / +inf / -inf, and a prior row with zeros, a NaN, a negative entry, and now and then no weight."""
    rows = leaves["rows"]
    rb = rows.shape[-1]
    wt = (torch.arange(rb, device=rows.device, dtype=torch.int64) * 2654435761 + 12345) % 1000003 + 1
    h = (rows.to(torch.int64) * wt).sum(-1) % 1000003                              # [R, P]
    value = (h.to(torch.float64) / 1000003.0 - 0.7) * 3.1
    value = torch.where(h % 17 == 0, torch.full_like(value, float("nan")), value)
    value = torch.where(h % 19 == 1, torch.full_like(value, float("inf")), value)
    value = torch.where(h % 23 == 2, torch.full_like(value, float("-inf")), value).contiguous()
    if not with_prior:
        return value, None
    col = torch.arange(K, device=rows.device, dtype=torch.int64)
    q = (h[..., None] * (col + 3) * 7919 + col * 104729) % 1013
    prior = q.to(torch.float32) / 1013.0
    prior = torch.where(q % 5 == 0, torch.zeros_like(prior), prior)
    prior = torch.where((h % 7 == 0)[..., None], torch.zeros_like(prior), prior)  # a row without weight: the block stays
    prior[..., 0] = torch.where(h % 11 == 3, torch.full_like(prior[..., 0], float("nan")), prior[..., 0])
    prior[..., K - 1] = torch.where(h % 13 == 4, torch.full_like(prior[..., 0], -2.0), prior[..., K - 1])
    return value, prior.contiguous()


def _session_both(b, n_waves, n_par, what, root_prior=None, leaf_priors=False, node_cap=None, group=None, max_sims=None):
    """A device session and the twin side by side under the synthetic evaluator: paths, leaf records, returns, visits, values, info and
    the best line compared after EVERY wave; the leaves compared with peek.  Returns (the last device result, all paths, the twin)."""
    K = max(b.k_max, 1)
    lo, hi = (0, b.n_envs) if group is None else b.group_bounds(group)
    rows = hi - lo
    M = n_waves * n_par if max_sims is None else max_sims
    cap = 1 + (M + 1) * K if node_cap is None else node_cap
    sess = et.Session(_legal_rows(b, lo, hi), n_par, cap, _lib.tree_exploration_table(1.25, 19652.0, M), M, K,
                      None if root_prior is None else root_prior.cpu().numpy().tolist())
    before = _snapshot(b)
    b.tree_open(n_par, M, root_prior, node_cap, group=group)
    res, all_paths = None, []
    for w in range(n_waves):
        lv = b.tree_leaves(group=group)
        value, prior = _synthetic(lv, K, leaf_priors)
        res = _np(b.tree_backup(value, prior, group=group))
        tp, tl = sess.leaves()
        _same(lv["paths"].cpu().numpy(), np.array(tp, np.int32).reshape(rows, n_par, K), (what, w, "paths"))
        _same(lv["leaf"].cpu().numpy(), np.array(tl, np.int32).reshape(rows, n_par, 2), (what, w, "leaf"))
        pk = b.peek(lv["paths"], group=group)
        for k in ("rows", "out", "ret"):
            assert lv[k].cpu().numpy().tobytes() == pk[k].cpu().numpy().tobytes(), (what, w, "peek", k)
        tres, tG = sess.backup(lv["ret"].cpu().numpy().tolist(), value.cpu().numpy().tolist(), None if prior is None else prior.cpu().numpy().tolist())
        tw = dict(visits=np.array([r["visits"] for r in tres], np.int32), value=np.array([r["value"] for r in tres], np.float64),
                  info=np.array([r["info"] for r in tres], np.int32), best_order=np.array([r["best_order"] for r in tres], np.int32),
                  best_return=np.array([r["best_return"] for r in tres], np.float64), returns=np.array(tG, np.float64).reshape(rows, n_par))
        for k in RESULT:
            _same(res[k], tw[k], (what, w, k))
        all_paths.append(lv["paths"].cpu().numpy())
    assert _snapshot(b) == before, what
    return res, np.concatenate(all_paths, axis=1), sess


# ---- 1. twin equivalence, bit for bit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_par", [1, 2, 5, 70])
def test_the_device_session_equals_the_twin_bit_for_bit_after_every_wave(n_par):
    regions = _mixed_regions()
    n = 24
    b = RegionBatch(regions, n_envs=n, device=DEV)
    b.reset()
    _advance(b, 2)
    K = b.k_max
    assert K <= 10
    waves = 4 if n_par < 70 else 3
    seen = {}
    for root in (False, True):
        for leafp in (False, True):
            res, paths, sess = _session_both(b, waves, n_par, (n_par, root, leafp), root_prior=_random_prior(n, K, 77 + n_par) if root else None,
                                             leaf_priors=leafp)
            seen[(root, leafp)] = paths
            live = np.array([bool(t.legal) for t in sess.trees])
            assert (res["info"][live, 0] == waves * n_par).all() and not res["info"][~live].any()
            assert (res["visits"].sum(axis=1)[live] == waves * n_par).all()
            if leafp:
                assert sum(t.repriored for t in sess.trees) > 0
    if n_par >= 5:          # the inputs bite (the twin alone says so): both priors change where the search goes, some lines end the episode
        assert not np.array_equal(seen[(False, False)], seen[(True, False)]) and not np.array_equal(seen[(False, False)], seen[(False, True)])
        assert max(t.max_depth for t in sess.trees) >= 3 and sum(t.terminal_visits for t in sess.trees) > 0 and sum(t.ties for t in sess.trees) > 0


# ---- 2. the anchor: values that complete every line to a rollout's return reproduce the rollout search --------------------------------
@pytest.mark.parametrize("n_par", [2, 5])
def test_values_from_rollouts_reproduce_tree_search_bit_for_bit(n_par):
    regions = _mixed_regions()
    n, W = 24, 4
    b = RegionBatch(regions, n_envs=n, device=DEV)          # the default reward weights: every reward is a multiple of 0.5, exact in double
    b.reset()
    _advance(b, 1)
    K = b.k_max
    cap = 1 + W * n_par * K
    want = _np(b.tree_search(W, n_par, SEED, node_cap=cap, trace=True))
    b.tree_open(n_par, W * n_par, None, cap)
    paths, returns = [], []
    for w in range(W):
        lv = b.tree_leaves()
        ro = b.rollout(n_par, _lib.tree_seed(SEED, w), prefix=lv["paths"])
        assert bool(((ro["ret"] * 2.0) == torch.round(ro["ret"] * 2.0)).all())
        res = b.tree_backup((ro["ret"] - lv["ret"]).contiguous(), None)
        paths.append(lv["paths"]); returns.append(res["returns"])
    got = _np(dict(res, paths=torch.cat(paths, dim=1), returns=torch.cat(returns, dim=1)))
    for k in ("visits", "value", "info", "paths", "returns"):
        _same(got[k], want[k], (n_par, k))
    assert (want["info"][:, 2] >= 2).any()


def test_wide_blocks_entered_within_their_wave_as_the_pool_runs_out_match_across_forms():
    """Blocks wider than a wavefront, made by one lane of a wave and entered by a later lane of the same wave, in a pool that runs out
    part-way: the rollout search and the evaluated session fed with rollout returns, bit for bit.  All the prior's weight is on two nets,
    so in wave 0 lane 0 takes the lowest net (E[0] == 0: a tie), lane 1 the heavier net, and lane 2 follows lane 1 into the block lane 1
    has just made; the pool holds the root, its block and those two blocks, so lane 2's own block is the one that does not fit.
    best_return is compared with what each form's spec says of it, not across the forms: with more than 128 legal nets and 6 simulations
    no line of the session ends the episode, so the session's best terminal line is -inf, while the rollout search's is its highest G."""
    from tests.helpers import OBS_MANY_NETS
    b = RegionBatch([generate_region(9300, **OBS_MANY_NETS)], n_envs=1, device=DEV)
    assert b.legal_words >= 4
    b.reset()
    nets = _legal_rows(b)[0]
    nlegal, K = len(nets), b.k_max
    assert nlegal > 128
    prior = torch.zeros((1, K), dtype=torch.float32, device=DEV)          # test_a_region_with_several_legal_words' prior
    prior[0, nets[-1] - 1] = 5.0
    prior[0, nets[70] - 1] = 1.0
    n_par, W = 3, 2
    cap = 1 + nlegal + 2 * (nlegal - 1)                                    # the root, its block, exactly two second-level blocks
    want = _np(b.tree_search(W, n_par, SEED, prior=prior, node_cap=cap, trace=True))
    b.tree_open(n_par, W * n_par, prior, cap)
    paths, returns = [], []
    for w in range(W):
        lv = b.tree_leaves()
        ro = b.rollout(n_par, _lib.tree_seed(SEED, w), prefix=lv["paths"])
        assert bool(((ro["ret"] * 2.0) == torch.round(ro["ret"] * 2.0)).all())
        res = b.tree_backup((ro["ret"] - lv["ret"]).contiguous(), None)
        paths.append(lv["paths"]); returns.append(res["returns"])
    got = _np(dict(res, paths=torch.cat(paths, dim=1), returns=torch.cat(returns, dim=1)))
    for k in ("visits", "value", "info", "paths", "returns"):
        _same(got[k], want[k], k)
    _same(want["best_return"], want["returns"].max(axis=1), "best_return, rollout search")
    assert (got["best_return"] == -np.inf).all()
    assert (want["info"][:, 3] == FULL).all() and (want["info"][:, 2] >= 2).all() and (want["info"][:, 1] == cap).all()
    assert ((want["paths"][0, 1:n_par] > 0).sum(axis=1) == 2).any()       # a later lane of wave 0 went through a block made in wave 0


# ---- 4. edges -----------------------------------------------------------------------------------------------------------------------
def test_a_region_with_more_than_64_nets():
    wide = generate_region(9400, dims=(23, 15, 5), k_range=(66, 70), net_span=6, pins=(2, 2), aps=(1, 1))
    b = RegionBatch([wide], n_envs=2, device=DEV)
    assert b.legal_words >= 2
    b.reset()
    b.step(torch.tensor([3, 0], dtype=torch.int32, device=DEV))          # the two rows differ
    nets = _legal_rows(b)
    assert len(nets[1]) > 64 and max(nets[1]) > 64                         # blocks wider than a wavefront, nets of the second word
    K = b.k_max
    prior = torch.zeros((2, K), dtype=torch.float32, device=DEV)
    prior[:, nets[1][-1] - 1] = 5.0                                        # the prior's favourite lives in the second word
    prior[:, nets[1][10] - 1] = 1.0
    res, paths, sess = _session_both(b, 3, 3, "wide, priors", root_prior=prior, leaf_priors=True)
    assert (res["info"][:, 0] == 9).all() and (res["info"][:, 3] == 0).all() and (res["info"][:, 1] > 1 + 64).all()
    assert paths[1, 0, 0] == nets[1][0] and paths[1, 1, 0] == nets[1][-1]  # E[0] == 0: a tie, the lowest net; then the heaviest prior
    assert sum(t.repriored for t in sess.trees) > 0
    _session_both(b, 2, 2, "wide, uniform")


def test_one_legal_net_done_envs_and_reopening_after_a_step():
    regions = [generate_region(9500 + i, dims=(10, 9, 4), k_range=(1 + i % 3, 1 + i % 3), net_span=5) for i in range(6)]
    b = RegionBatch(regions, device=DEV, auto_reset=False)
    b.reset()
    nl = b.fetch("nlegal").cpu().numpy()
    assert set(nl.tolist()) == {1, 2, 3}
    res, paths, sess = _session_both(b, 3, 2, "1..3 nets", leaf_priors=True)
    one = nl == 1
    assert (res["info"][one, 1] == 2).all() and (res["info"][one, 2] == 1).all() and all(sess.trees[i].terminal_visits >= 5 for i in np.flatnonzero(one))
    b.tree_open(2, 6)
    lv = b.tree_leaves()                                                   # a session left open with pending leaves ...
    b.step(b.random_actions(SEED))                                         # ... and the env steps: the caller must re-open, and does
    nl = b.fetch("nlegal").cpu().numpy()
    assert (nl == 0).sum() == 2 and (nl > 0).sum() == 4
    res, paths, sess = _session_both(b, 3, 2, "after a step", leaf_priors=True)
    done = nl == 0
    assert not res["visits"][done].any() and not res["info"][done].any() and not res["best_order"][done].any() and not paths[done].any()
    assert (res["value"][done] == -np.inf).all() and (res["best_return"][done] == -np.inf).all() and (res["returns"][done].view(np.uint64) == 0).all()
    assert (res["info"][~done, 0] == 6).all()


@pytest.mark.parametrize("cap", ["one", "root block"])
def test_full_pools(cap):
    regions = [generate_region(9400, dims=(14, 12, 4), k_range=(5, 5), net_span=5)]
    b = RegionBatch(regions, n_envs=6, device=DEV)
    b.reset()
    k = int(b.fetch("nlegal").cpu().numpy()[0])
    assert k >= 3
    if cap == "one":
        res, paths, _ = _session_both(b, 2, 4, "node_cap 1", node_cap=1, leaf_priors=True)
        assert not paths.any() and not res["visits"].any() and (res["value"] == -np.inf).all()
        assert (res["info"] == np.array([8, 1, 0, FULL], np.int32)).all() and (res["best_return"] == -np.inf).all()
    else:
        res, paths, _ = _session_both(b, 3, 4, "node_cap K + 1", node_cap=k + 1, leaf_priors=True)
        assert (res["info"] == np.array([12, k + 1, 1, FULL], np.int32)).all() and (res["visits"].sum(axis=1) == 12).all()
        assert ((paths > 0).sum(axis=2) == 1).all()


def test_call_order_and_max_sims_on_a_live_batch():
    regions = [generate_region(3000 + i, dims=(12, 10, 4), k_range=(3, 6)) for i in range(4)]
    b = RegionBatch(regions, device=DEV)
    b.reset()
    K = b.k_max
    STATE, RANGE = _lib.XR_ERR_STATE, _lib.XR_ERR_RANGE
    before = _snapshot(b)
    zero = torch.zeros((4, 2), dtype=torch.float64, device=DEV)

    def refused(fn, code, word):
        with pytest.raises(_lib.XRouteError) as ei:
            fn()
        assert ei.value.code == code and word in str(ei.value), ei.value

    b._tree_sessions = {-1: 2}                                             # (past Python's own check: the library's refusals)
    refused(lambda: b.tree_leaves(), STATE, "xr_batch_tree_leaves")
    refused(lambda: b.tree_backup(zero), STATE, "xr_batch_tree_backup")
    b.tree_open(2, 5)                                                      # room for two waves of two, not for three
    refused(lambda: b.tree_backup(zero), STATE, "xr_batch_tree_backup")
    first = b.tree_leaves()
    refused(lambda: b.tree_leaves(), STATE, "xr_batch_tree_leaves")
    b.tree_backup(zero)
    b.tree_leaves()
    res = _np(b.tree_backup(zero))
    refused(lambda: b.tree_leaves(), RANGE, "max_sims")
    refused(lambda: b.tree_backup(zero), STATE, "xr_batch_tree_backup")    # nothing is pending after the refusal
    assert (res["info"][:, 0] == 4).all() and _snapshot(b) == before
    for bad, word in ((dict(n_par=0, max_sims=4), "n_par"), (dict(n_par=4, max_sims=3), "max_sims"), (dict(n_par=2, max_sims=4, node_cap=0), "node_cap")):
        with pytest.raises(ValueError, match=word):
            b.tree_open(**bad)
    # a new open starts over: its first wave is the first session's first wave
    b.tree_open(2, 5)
    again = b.tree_leaves()
    assert torch.equal(again["paths"], first["paths"]) and torch.equal(again["leaf"], first["leaf"])
    b.tree_backup(zero)
    b.step(b.random_actions(SEED + 1))            # still usable


@pytest.mark.parametrize("kw", [dict(force_scratch_field=True), dict(stream_per_region=True)])
def test_the_scratch_forms_are_refused_and_the_batch_is_untouched(kw):
    regions = [generate_region(3000 + i, dims=(12, 10, 4), k_range=(3, 6)) for i in range(4)]
    b = RegionBatch(regions, device=DEV, **kw)
    b.reset()
    before = _snapshot(b)
    with pytest.raises(_lib.XRouteError) as ei:
        b.tree_open(2, 4)
    assert ei.value.code == _lib.XR_ERR_RANGE and "xr_batch_tree_open" in str(ei.value)
    assert _snapshot(b) == before


# ---- 5. coexistence -----------------------------------------------------------------------------------------------------------------
def test_a_kept_tree_and_a_plain_search_interleaved_with_a_session_give_their_stand_alone_results():
    regions = _mixed_regions()
    kw = dict(n_envs=24, device=DEV)
    a, t = RegionBatch(regions, **kw), RegionBatch(regions, **kw)
    a.reset(); t.reset()
    _advance(a, 1); _advance(t, 1)
    K = a.k_max
    still = torch.zeros(24, dtype=torch.int32, device=DEV)
    # stand-alone, each on its own
    kept1 = _np(t.tree_search(2, 3, SEED, keep=True, trace=True))
    kept2 = _np(t.tree_search(2, 3, SEED + 1, keep=True, played=still, trace=True))
    plain = _np(t.tree_search(3, 2, SEED + 2, trace=True))
    alone, alone_paths, _ = _session_both(t, 3, 3, "stand-alone", leaf_priors=True)
    # interleaved
    before = _snapshot(a)
    got_kept1 = _np(a.tree_search(2, 3, SEED, keep=True, trace=True))
    a.tree_open(3, 9)
    waves, paths = [], []
    for w in range(3):
        lv = a.tree_leaves()
        if w == 0:
            got_plain = _np(a.tree_search(3, 2, SEED + 2, trace=True))
        if w == 1:
            got_kept2 = _np(a.tree_search(2, 3, SEED + 1, keep=True, played=still, trace=True))
        value, prior = _synthetic(lv, K, True)
        if w == 2:
            a.rollout(2, SEED)                                             # (and the pool the peek launch shares)
        waves.append(_np(a.tree_backup(value, prior)))
        paths.append(lv["paths"].cpu().numpy())
    assert _snapshot(a) == before
    for k in kept1:
        _same(got_kept1[k], kept1[k], ("kept 1", k)); _same(got_kept2[k], kept2[k], ("kept 2", k))
    for k in plain:
        _same(got_plain[k], plain[k], ("plain", k))
    for k in RESULT:
        _same(waves[-1][k], alone[k], ("session", k))
    _same(np.concatenate(paths, axis=1), alone_paths, "session paths")
    assert (got_kept2["kept"][:, 0] > 0).any()


# ---- 6. groups ----------------------------------------------------------------------------------------------------------------------
def test_two_groups_on_two_streams_interleaved_equal_the_sessions_run_one_after_the_other():
    regions = _mixed_regions()
    kw = dict(n_envs=24, device=DEV)
    a, t = RegionBatch(regions, **kw), RegionBatch(regions, **kw)
    a.set_groups([0, 10, 24]); t.set_groups([0, 10, 24])
    a.reset(); t.reset()
    _advance(a, 1); _advance(t, 1)
    K = a.k_max
    shape = {0: (3, 2), 1: (2, 4)}                                          # (waves, lanes) differ between the groups
    want = {g: _session_both(t, shape[g][0], shape[g][1], ("alone", g), leaf_priors=True, root_prior=_random_prior(t.group_bounds(g)[1] - t.group_bounds(g)[0], K, g),
                             group=g) for g in (0, 1)}
    torch.cuda.synchronize()
    cur = torch.cuda.current_stream()
    streams = [torch.cuda.Stream() for _ in range(2)]
    priors = [_random_prior(a.group_bounds(g)[1] - a.group_bounds(g)[0], K, g) for g in (0, 1)]
    torch.cuda.synchronize()
    last, paths = {}, {0: [], 1: []}
    for g in (0, 1):
        streams[g].wait_stream(cur)
        with torch.cuda.stream(streams[g]):
            a.tree_open(shape[g][1], shape[g][0] * shape[g][1], priors[g], group=g, stream=streams[g])
    for w in range(3):
        lv = {}
        for g in (0, 1):
            if w < shape[g][0]:
                with torch.cuda.stream(streams[g]):
                    lv[g] = a.tree_leaves(group=g, stream=streams[g])
        for g in (1, 0):
            if w < shape[g][0]:
                with torch.cuda.stream(streams[g]):
                    value, prior = _synthetic(lv[g], K, True)
                    last[g] = a.tree_backup(value, prior, group=g, stream=streams[g])
                    paths[g].append(lv[g]["paths"])
    for s in streams:
        cur.wait_stream(s)
    torch.cuda.synchronize()
    for g in (0, 1):
        res, all_paths, _ = want[g]
        got = _np(last[g])
        for k in RESULT:
            _same(got[k], res[k], (g, k))
        _same(torch.cat(paths[g], dim=1).cpu().numpy(), all_paths, (g, "paths"))


def test_vector_env_sessions_whole_batch_and_group():
    from xroute_env_amd.envs.vector_env import XRouteVectorEnv
    regions = _mixed_regions()
    env = XRouteVectorEnv(regions, n_envs=24, device=DEV, max_route_count=1, groups=3, with_observation=False)
    env.reset()
    K = env.batch.k_max
    env.tree_open(2, 4)
    lv = env.tree_leaves()
    value, prior = _synthetic(lv, K, True)
    whole = _np(env.tree_backup(value, prior))
    lo, hi = env.batch.group_bounds(1)
    env.tree_open(2, 4, group=1)
    lg = env.tree_leaves(group=1)
    env.step_wait(1)
    assert torch.equal(lg["paths"], lv["paths"][lo:hi]) and torch.equal(lg["rows"], lv["rows"][lo:hi])
    part = env.tree_backup(value[lo:hi].contiguous(), prior[lo:hi].contiguous(), group=1)
    env.step_wait(1)
    torch.cuda.synchronize()
    for k in RESULT:
        _same(_np(part)[k], whole[k][lo:hi], k)


# ---- 7. the evaluators --------------------------------------------------------------------------------------------------------------
def _model():
    from xroute_env_amd.agents import ActorCritic
    torch.manual_seed(7)
    return ActorCritic(device=DEV).to(DEV).eval()


def test_critic_and_actor_critic_evaluators_on_the_ispd18_pack():
    from tests.test_gpu_peek import _Twin
    from xroute_env_amd.agents import GroupedFusedPolicy
    from xroute_env_amd.envs import peek as pk
    from xroute_env_amd.envs.tree_eval import actor_critic_evaluator, critic_evaluator, evaluated_search
    regions = _pack(slice(5, 200, 13))[:8]
    n, P = 8, 3
    b = RegionBatch(regions, n_envs=n, device=DEV, auto_reset=False)
    b.reset()
    _advance(b, 2)
    model = _model()
    pol = GroupedFusedPolicy(model, b)
    towers = {shape: tw for shape, tw in zip(pol.shapes, pol.towers) if tw is not None}
    groups = pk.shape_groups(b)
    K = b.k_max
    critic = critic_evaluator(model, towers, groups)
    both = actor_critic_evaluator(model, pol, groups)
    b.tree_open(P, 3 * P)
    twin = _Twin(regions, n)
    sd = b.state_dict()
    every = torch.arange(n, device=DEV)
    fresh_seen = 0
    for w in range(3):
        lv = b.tree_leaves()
        value, none = critic(b, lv)
        value2, prior = both(b, lv)
        assert none is None and value.dtype == torch.float64 and tuple(value.shape) == (n, P) and prior.dtype == torch.float32 and tuple(prior.shape) == (n, P, K)
        # the same heads from twins stepped along every lane's path, then the same function on the same pieces: test_gpu_peek.py's comparison (exact)
        paths = lv["paths"].cpu().numpy()
        heads = torch.zeros((n, P, 2 * b.n_max), dtype=torch.float32, device=DEV)
        legal_after = np.zeros((n, P, K), bool)
        for j in range(P):
            heads[:, j] = torch.from_numpy(twin.after(sd, paths[:, j])["head"]).to(DEV)
            legal_after[:, j] = np.array([[net in row for net in range(1, K + 1)] for row in _legal_rows(twin.t)])
        want = torch.zeros((n, P), dtype=torch.float64, device=DEV)
        for dims, idx in groups:
            idx = every if idx is None else idx
            v = pk.state_values(model, heads.index_select(0, idx).reshape(idx.numel() * P, -1), dims, towers).to(torch.float64).reshape(idx.numel(), P)
            want.index_copy_(0, idx, v)
        assert torch.equal(value, want), (w, (value - want).abs().max().item())
        assert torch.equal(value2, want), (w, (value2 - want).abs().max().item())
        # the prior: a distribution over the leaf state's legal nets, 0 elsewhere
        p = prior.cpu().numpy()
        assert np.isfinite(p).all() and (p >= 0).all() and not p[~legal_after].any()
        assert np.allclose(p.sum(-1), legal_after.any(-1).astype(np.float32), atol=1e-5)
        assert (p[legal_after] > 0).all()
        fresh_seen += int((lv["leaf"][..., 1] & FRESH).bool().sum())
        b.tree_backup(value2, prior)
    assert fresh_seen > 0
    twin.close()
    res = evaluated_search(b, both, 2, P, trace=True)
    live = b.fetch("nlegal") > 0
    assert tuple(res["paths"].shape) == (n, 2 * P, K) and int(live.sum()) >= 4
    assert bool((res["info"][live, 0] == 2 * P).all()) and not bool(res["info"][~live].any())


# ---- 8. whole episodes --------------------------------------------------------------------------------------------------------------
def test_evaluated_episodes_end_every_region_and_replay_on_the_oracle():
    from oracle import xr_oracle as orc
    from xroute_env_amd.envs.tree_eval import evaluated_episodes
    regions = _mixed_regions()[:4]

    def evaluate(batch, leaves, group=None, stream=None):
        return _synthetic(leaves, max(batch.k_max, 1), True)

    stats = {}
    out = evaluated_episodes(regions, evaluate, 3, 4, device=DEV, stats=stats)
    assert len(out) == 4 and stats["routed_nets"] > 0 and stats["plies"] == sum(r.n_nets for r in regions)
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
        assert env.nlegal() == 0 and tot == o["ret"]                                  # every region ends done
        assert o["best_ret"] >= o["ret"] and o["simulations"] == 12 * len(o["order"])
