"""Kept evaluated trees (xr_batch_tree_reopen, "XR-Tree v2, kept") on the GPU: the device session against the spec's twin
(tests/tree_eval_keep_twin.py) under the synthetic, state-dependent evaluator of tests/test_gpu_tree_eval.py, bit for bit after every
wave (doubles compared as uint64), with the batch snapshot unchanged around every session — a fresh reopen against tree_open, whole
episodes of search -> step the most visited net -> reopen, played == 0, every rebuild case, the simulation budget, an exactly filled
pool, purity, coexistence with the other pools, groups on streams, refusals, the vector env and evaluated_episodes(reuse=True).

Shapes: tests/test_gpu_tree_keep.py's small regions (grids of (12, 10, 4) with 1, 2, 5, 5 and 3 nets) and its wide ones (one (23, 15,
5) region with 65-70 nets: two legal words, a root block wider than a wavefront); n_par in {1, 3}, up to 4 waves."""
import gc

import numpy as np
import pytest
import torch

from tests import test_gpu_tree_eval as te
from tests import test_gpu_tree_keep as tk
from tests import tree_eval_keep_twin as ekt
from xroute_env_amd import _lib
from xroute_env_amd.batch import RegionBatch
from xroute_env_amd.envs.vector_env import XRouteVectorEnv
from xroute_env_amd.regions import generate_region

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x2EE7
KEPT, FULL = _lib.XR_TREE_KEPT, _lib.XR_TREE_POOL_FULL
MAX_SIMS = _lib.XR_TREE_MAX_SIMS
RESULT = te.RESULT
WAVE = ("paths", "leaf", "rows", "out", "ret") + RESULT
_same, _np, _snapshot, _states, _synthetic = te._same, te._np, te._snapshot, tk._states, te._synthetic


@pytest.fixture(autouse=True)
def _release_cached_memory():
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _prior(rows, K, seed):
    return te._random_prior(rows, K, seed)


def _act(res):
    return tk._act({k: res[k] for k in ("visits", "value", "best_order")})


def _waves(b, n_waves, n_par, opener, leaf_priors=True, group=None):
    """A device session on its own: opener() starts it; every output of every wave, as numpy."""
    K = max(b.k_max, 1)
    kept = opener()
    out = []
    for _ in range(n_waves):
        lv = b.tree_leaves(group=group)
        value, prior = _synthetic(lv, K, leaf_priors)
        res = b.tree_backup(value, prior, group=group)
        out.append(_np(dict(lv, **res)))
    return out, None if kept is None else kept.cpu().numpy()


class Pair:
    """The evaluated-tree pool of one caller of `b` (the whole batch, or a group) on the device and in the twin, side by side."""

    def __init__(self, b, group=None):
        self.b, self.group, self.pool = b, group, ekt.KeyedPool()
        self.lo, self.hi = (0, b.n_envs) if group is None else b.group_bounds(group)

    def run(self, played, n_waves, n_par, node_cap, what, root_prior=None, leaf_priors=False, max_sims=None, c_init=1.25, c_base=19652.0, backup_last=True):
        """One keyed session: reopen, then n_waves waves; kept, paths, leaf records, returns, visits, values, info and the best line
        compared after EVERY wave; the batch untouched.  backup_last=False abandons the last wave after its leaves.  Returns (the last
        device result with `kept` and all `paths`, the twin's session)."""
        b, g, K, rows = self.b, self.group, max(self.b.k_max, 1), self.hi - self.lo
        M = n_waves * n_par if max_sims is None else max_sims
        before = _snapshot(b)
        kept = b.tree_open(n_par, M, root_prior, node_cap, c_init, c_base, group=g, keep=True, played=played).cpu().numpy()
        sess, tkept = self.pool.reopen(_states(b, self.lo, self.hi), None if played is None else played.cpu().numpy().tolist(), n_par, node_cap,
                                       tk._E(c_init, c_base), M, K, None if root_prior is None else root_prior.cpu().numpy().tolist(), lo=self.lo,
                                       legal_words=b.legal_words)
        _same(kept, np.array(tkept, np.int32).reshape(rows, 2), (what, "kept"))
        res, all_paths = None, []
        for w in range(n_waves):
            lv = b.tree_leaves(group=g)
            tp, tl = sess.leaves()
            _same(lv["paths"].cpu().numpy(), np.array(tp, np.int32).reshape(rows, n_par, K), (what, w, "paths"))
            _same(lv["leaf"].cpu().numpy(), np.array(tl, np.int32).reshape(rows, n_par, 2), (what, w, "leaf"))
            all_paths.append(lv["paths"].cpu().numpy())
            if w == n_waves - 1 and not backup_last:
                break
            value, prior = _synthetic(lv, K, leaf_priors)
            res = _np(b.tree_backup(value, prior, group=g))
            tres, tG = sess.backup(lv["ret"].cpu().numpy().tolist(), value.cpu().numpy().tolist(), None if prior is None else prior.cpu().numpy().tolist())
            tw = dict(visits=np.array([r["visits"] for r in tres], np.int32), value=np.array([r["value"] for r in tres], np.float64),
                      info=np.array([r["info"] for r in tres], np.int32), best_order=np.array([r["best_order"] for r in tres], np.int32),
                      best_return=np.array([r["best_return"] for r in tres], np.float64), returns=np.array(tG, np.float64).reshape(rows, n_par))
            for k in RESULT:
                _same(res[k], tw[k], (what, w, k))
        assert _snapshot(b) == before, what
        return (None if res is None else dict(res, kept=kept, paths=np.concatenate(all_paths, axis=1))), sess


# ---- 1. a fresh reopen is tree_open --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_par", [1, 3])
@pytest.mark.parametrize("regions", ["small", "wide"])
def test_a_fresh_reopen_equals_open_and_leaves_the_next_open_unchanged(regions, n_par):
    b = RegionBatch(tk._small_regions() if regions == "small" else tk._wide_regions(), device=DEV)
    b.reset()
    K, n, W = b.k_max, b.n_envs, 4
    M = W * n_par
    cap = 1 + (M + 1) * K
    prior = _prior(n, K, 31)
    want, none = _waves(b, W, n_par, lambda: b.tree_open(n_par, M, prior, cap))
    got, kept = _waves(b, W, n_par, lambda: b.tree_open(n_par, M, prior, cap, keep=True))
    again, _ = _waves(b, W, n_par, lambda: b.tree_open(n_par, M, prior, cap))
    assert none is None and kept.shape == (n, 2) and not kept.any()
    for w in range(W):
        for k in WAVE:
            _same(got[w][k], want[w][k], (regions, n_par, "reopen vs open", w, k))
            _same(again[w][k], want[w][k], (regions, n_par, "open again", w, k))
        assert not (got[w]["info"][:, 3] & KEPT).any()
    assert (want[-1]["info"][:, 0] == M).all()
    if regions == "wide":
        assert b.fetch("nlegal").cpu().numpy()[0] > 64 and b.legal_words >= 2


# ---- 2. whole episodes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("priors", [False, True])
def test_an_episode_of_search_step_reopen_equals_the_twin_at_every_wave_of_every_ply(priors):
    b = RegionBatch(tk._small_regions(), device=DEV, auto_reset=False)
    b.reset()
    K, n = b.k_max, b.n_envs
    pair = Pair(b)
    cap = 1 + 4 * (12 + 1) * K
    played, kept_plies, repriored = None, 0, 0
    for ply in range(K + 1):
        nl = b.fetch("nlegal").cpu().numpy()
        if not (nl > 0).any():
            break
        dev, sess = pair.run(played, 4, 3, cap, ("episode", priors, ply), root_prior=_prior(n, K, 100 + ply) if priors else None, leaf_priors=priors)
        repriored += sum(t.repriored for t in sess.trees)
        if played is not None:
            must = (nl > 0) & (played.cpu().numpy() > 0)          # stepped with the root's most visited child, and a net is left
            assert ((dev["info"][must, 3] & KEPT) != 0).all(), ply
            assert (dev["kept"][must, 1] >= 1 + nl[must]).all(), (ply, dev["kept"][must].tolist(), nl[must].tolist())
            # the carried visits are in the root's counts, but for the one that stopped at the child while it was a leaf
            assert (dev["visits"].sum(axis=1)[must] == dev["kept"][must, 0] - 1 + 12).all(), ply
            assert (dev["info"][must, 0] == 12).all()
            kept_plies += int(must.any())
        act = _act(dev)
        b.step(act)
        played = act
    assert kept_plies >= 4 and not (b.fetch("nlegal") > 0).any()
    assert (repriored > 0) == priors          # (the evaluator's priors reached blocks that later sessions carried)


# ---- 3. blocks wider than a wavefront ------------------------------------------------------------------------------------------------
def test_three_plies_of_a_region_whose_blocks_are_wider_than_a_wavefront():
    b = RegionBatch(tk._wide_regions(), device=DEV, auto_reset=False)
    b.reset()
    K = b.k_max
    assert b.fetch("nlegal").cpu().numpy()[0] > 64 and b.legal_words >= 2
    pair = Pair(b)
    cap = 1 + 40 * K
    played = None
    for ply in range(3):
        dev, _ = pair.run(played, 4, 3, cap, ("wide", ply), leaf_priors=bool(ply & 1))
        if ply:
            assert dev["info"][0, 3] == KEPT and dev["kept"][0, 1] > 64, dev["kept"][0].tolist()          # a block above 64 nodes was copied
        act = _act(dev)
        b.step(act)
        played = act


# ---- 4. the env has not moved --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_par", [1, 3])
def test_played_zero_adds_simulations_to_the_same_root(n_par):
    b = RegionBatch(tk._small_regions(), device=DEV, auto_reset=False)
    b.reset()
    pair = Pair(b)
    cap = 1 + 8 * n_par * b.k_max
    zero = torch.zeros(b.n_envs, dtype=torch.int32, device=DEV)
    first, _ = pair.run(None, 2, n_par, cap, "first half", leaf_priors=True)
    second, sess = pair.run(zero, 2, n_par, cap, "second half", leaf_priors=True)
    assert (second["info"][:, 3] == KEPT).all() and (second["kept"][:, 0] == 2 * n_par).all()
    assert np.array_equal(second["kept"][:, 1], first["info"][:, 1])
    assert (second["visits"].sum(axis=1) == 4 * n_par).all() and all(t.nodes[0].N == 4 * n_par for t in sess.trees)
    assert (second["info"][:, 0] == 2 * n_par).all()
    # max_sims, the knobs and the prior may differ: still kept
    third, _ = pair.run(zero, 1, n_par, cap, "third", max_sims=5 * n_par, c_init=0.5, c_base=100.0, root_prior=_prior(b.n_envs, b.k_max, 9))
    assert (third["info"][:, 3] & KEPT).all() and (third["kept"][:, 0] == 4 * n_par).all()


# ---- 5. rebuilds ---------------------------------------------------------------------------------------------------------------------
def _fresh_rows(b, dev, rows, n_waves, n_par, cap, what, all_rows=False):
    """The rows `rows` of a keyed session equal a fresh session of the state the batch is in; the other live rows are kept."""
    M = n_waves * n_par
    fresh, _ = _waves(b, n_waves, n_par, lambda: b.tree_open(n_par, M, None, cap), leaf_priors=False)
    rows = np.array(rows)
    for k in RESULT:
        _same(dev[k][rows], fresh[-1][k][rows], (what, k))
    _same(dev["paths"][rows], np.concatenate([f["paths"] for f in fresh], axis=1)[rows], (what, "paths"))
    assert not dev["kept"][rows].any() and not (dev["info"][rows, 3] & KEPT).any(), what
    others = np.setdiff1d(np.flatnonzero(b.fetch("nlegal").cpu().numpy() > 0), rows)
    if all_rows:
        assert not len(others), what
    else:
        assert len(others) and (dev["info"][others, 3] & KEPT).all(), what


def _started(groups=None, **kw):
    b = RegionBatch(tk._small_regions()[2:] + tk._small_regions()[2:4], device=DEV, **kw)          # 5, 5, 3, 5, 5 nets
    if groups:
        b.set_groups(groups)
    b.reset()
    pair = Pair(b)
    cap = 1 + 4 * 7 * b.k_max
    dev, _ = pair.run(None, 2, 3, cap, "start")
    return b, pair, cap, _act(dev)


def test_a_wrong_net_and_a_negative_entry_rebuild_their_rows():
    b, pair, cap, act = _started()
    b.step(act)
    played = act.clone()
    played[1] = _states(b)[1].legal[0]                          # a net that was legal and was not the one played
    played[3] = -7
    dev, _ = pair.run(played, 2, 3, cap, "wrong net")
    _fresh_rows(b, dev, [1, 3], 2, 3, cap, "wrong net")


def test_envs_not_stepped_and_stepped_twice_rebuild_their_rows():
    b, pair, cap, act = _started(groups=[0, 2, 3, 5])
    b.step_group(0, act[0:2].contiguous())                      # group 0: one step; group 1: none; group 2: two
    b.step_group(2, act[3:5].contiguous())
    b.step_group(2, b.random_actions_group(2, SEED))
    torch.cuda.synchronize()
    dev, _ = pair.run(act, 2, 3, cap, "no step, two steps")
    _fresh_rows(b, dev, [2, 3, 4], 2, 3, cap, "no step, two steps")


def test_an_auto_reset_between_the_sessions_rebuilds_the_row():
    regs = tk._small_regions()
    b = RegionBatch([regs[0], regs[2], regs[3]], device=DEV, auto_reset=True, max_route_count=1)          # 1, 5, 5 nets
    b.reset()
    pair = Pair(b)
    cap = 1 + 4 * 7 * b.k_max
    played, seen = None, []
    for ply in range(3):
        dev, _ = pair.run(played, 2, 3, cap, ("auto reset", ply))
        seen.append((dev["info"][0].tolist(), dev["kept"][0].tolist()))
        act = _act(dev)
        b.step(act)
        played = act
    # row 0: a fresh tree, then a done row (its only net was played), then — the env has reset under it — a fresh tree again
    assert seen[0][0][0] == 6 and seen[1] == ([0, 0, 0, 0], [0, 0]) and seen[2][0][0] == 6 and seen[2][0][3] == 0 and seen[2][1] == [0, 0]
    assert (dev["info"][1:, 3] == KEPT).all()


def test_a_branch_from_a_slot_of_another_region_rebuilds_the_row():
    b, pair, cap, act = _started()
    b.step(act)
    b.branch(torch.tensor([0, 1, 1, 3, 4], dtype=torch.int32, device=DEV))          # slot 2 (3 nets) takes slot 1's state (another region)
    dev, _ = pair.run(act, 2, 3, cap, "branch")
    _fresh_rows(b, dev, [2], 2, 3, cap, "branch")


@pytest.mark.parametrize("change", ["node_cap", "n_par"])
def test_a_changed_shape_rebuilds_every_row(change):
    b, pair, cap, act = _started()
    b.step(act)
    cap2, par2 = (cap + 1, 3) if change == "node_cap" else (cap, 2)
    dev, _ = pair.run(act, 2, par2, cap2, change)
    assert not dev["kept"].any() and not (dev["info"][:, 3] & KEPT).any()
    act = _act(dev)
    b.step(act)
    dev, _ = pair.run(act, 2, par2, cap2, "the same shape again")
    assert (dev["info"][:, 3] & KEPT).all()
    _fresh_rows(b, pair.run(None, 2, par2, cap2, "played None")[0], list(range(b.n_envs)), 2, par2, cap2, "played None", all_rows=True)


def test_a_session_abandoned_after_its_leaves_forfeits_the_tree():
    b, pair, cap, act = _started()
    b.step(act)
    none, _ = pair.run(act, 1, 3, cap, "abandoned", backup_last=False)
    assert none is None
    zero = torch.zeros(b.n_envs, dtype=torch.int32, device=DEV)
    dev, _ = pair.run(zero, 2, 3, cap, "after the abandoned wave")
    _fresh_rows(b, dev, list(range(b.n_envs)), 2, 3, cap, "after the abandoned wave", all_rows=True)


def test_a_tree_open_in_between_rebuilds_every_row():
    b, pair, cap, act = _started()
    b.step(act)
    b.tree_open(3, 6, None, cap)
    pair.pool.open([s.legal for s in _states(b)], 3, cap, tk._E(), 6, b.k_max)
    dev, _ = pair.run(act, 2, 3, cap, "after an open session")
    _fresh_rows(b, dev, list(range(b.n_envs)), 2, 3, cap, "after an open session", all_rows=True)


# ---- 6. the simulation budget --------------------------------------------------------------------------------------------------------
def test_the_simulation_budget_keeps_at_exactly_the_limit_and_rebuilds_one_above():
    b = RegionBatch(tk._small_regions()[2:4], device=DEV, auto_reset=False)
    b.reset()
    pair = Pair(b)
    cap = 400
    zero = torch.zeros(2, dtype=torch.int32, device=DEV)
    pair.run(None, 2, 3, cap, "six simulations")
    dev, _ = pair.run(zero, 1, 3, cap, "N + max_sims == XR_TREE_MAX_SIMS", max_sims=MAX_SIMS - 6)
    assert (dev["kept"][:, 0] == 6).all() and (dev["info"][:, 3] == KEPT).all() and (dev["info"][:, 0] == 3).all()
    dev, _ = pair.run(zero, 1, 3, cap, "one above", max_sims=MAX_SIMS - 9 + 1)
    assert not dev["kept"].any() and not (dev["info"][:, 3] & KEPT).any()
    # and below the played child: its N is the root's visit count of that net
    dev, _ = pair.run(None, 2, 3, cap, "six simulations again")
    act = _act(dev)
    n_child = dev["visits"][np.arange(2), act.cpu().numpy() - 1]
    b.step(act)
    lim = int(n_child.min())
    dev, _ = pair.run(act, 1, 3, cap, "the played child's N", max_sims=MAX_SIMS - lim)
    assert ((dev["kept"][:, 0] > 0) == (n_child == lim)).all() and (dev["kept"][n_child == lim, 0] == lim).all()


# ---- 7. a pool filled to the last node -----------------------------------------------------------------------------------------------
def test_a_pool_the_continued_tree_fills_exactly_and_one_more_simulation_overflows():
    def run(cap, waves2):
        b = RegionBatch(tk._small_regions()[2:4], device=DEV, auto_reset=False)          # two rows of 5 nets; a batch of its own per run: the same state
        b.reset()
        pair = Pair(b)
        dev, _ = pair.run(None, 3, 1, cap, ("first", cap))
        act = _act(dev)
        b.step(act)
        return pair.run(act, waves2, 1, cap, ("second", cap, waves2))[0]
    roomy = run(1000, 6)
    cap = int(roomy["info"][0, 1])
    assert roomy["kept"][0, 1] < cap and roomy["info"][0, 3] == KEPT
    exact = run(cap, 6)
    assert exact["info"][0].tolist() == [6, cap, roomy["info"][0, 2], KEPT]          # full to the last node, and nobody has noticed
    for k in RESULT + ("paths", "kept"):
        _same(exact[k][:1], roomy[k][:1], ("exact", k))
    assert run(1000, 7)["info"][0, 1] > cap                                          # (the seventh simulation makes a block)
    over = run(cap, 7)
    assert over["info"][0, :2].tolist() == [7, cap] and over["info"][0, 3] == KEPT | FULL


# ---- 8. purity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])
def test_reopen_sessions_leave_the_batch_and_its_in_place_observation_alone(dtype):
    regs = tk._small_regions()
    kw = dict(n_envs=6, device=DEV, auto_reset=True, max_route_count=1)
    a, t = RegionBatch(regs, **kw), RegionBatch(regs, **kw)
    a.reset(); t.reset()
    K = a.k_max
    obs_a, obs_t = a.alloc_observation(dtype=dtype).zero_(), t.alloc_observation(dtype=dtype).zero_()
    a.observation(obs_a); t.observation(obs_t)
    played = None
    for step in range(6):
        before = _snapshot(a)
        waves, kept = _waves(a, 2, 3, lambda: a.tree_open(3, 6, None, 200, keep=True, played=played))
        res = waves[-1]
        assert step == 0 or bool((res["info"][:, 3] & KEPT).any())
        _waves(a, 1, 3, lambda: a.tree_open(3, 3, None, 200, keep=True, played=torch.zeros(6, dtype=torch.int32, device=DEV)))
        after = _snapshot(a)
        for k in before:
            assert before[k] == after[k], (step, k)
        act = _act(res)
        a.step(act, obs_a, inplace=True)
        t.step(act, obs_t, inplace=True)
        info = a.observe_info()
        assert info["form"] == 3 and info["inplace"], (step, info)          # the in-place path survived the sessions
        assert torch.equal(obs_a, obs_t), step
        for k in ("hash", "record", "owner", "legal", "env_steps"):
            assert a.fetch(k).cpu().numpy().tobytes() == t.fetch(k).cpu().numpy().tobytes(), (step, k)
        played = act


# ---- 9. pools apart ------------------------------------------------------------------------------------------------------------------
def test_a_keyed_tree_a_v1_kept_tree_and_a_plain_search_interleaved_give_their_stand_alone_results():
    b, pair, cap, act = _started(groups=[0, 2, 5])
    v1 = tk.Twin(b)
    g1 = Pair(b, group=1)
    kcap = 1 + 4 * 2 * 3 * b.k_max
    kdev, _ = tk._both(b, v1, None, 2, 3, SEED, kcap, "v1 kept, start")
    b.tree_search(2, 2, SEED + 2, node_cap=kcap)
    g1.run(None, 1, 3, cap, "group 1, start")
    kact = tk._act(kdev)
    b.step(act)                                                  # the keyed tree's most visited nets
    plain = _np(b.tree_search(2, 2, SEED + 3, node_cap=kcap, trace=True))
    dev, _ = pair.run(act, 2, 3, cap, "whole batch, continued", leaf_priors=True)
    tk._both(b, v1, kact, 2, 3, SEED + 1, kcap, "v1 kept, continued")          # (rows whose kept tree played another net are rebuilt: the twin says which)
    dev_g, _ = g1.run(act[2:5].contiguous(), 2, 3, cap, "group 1, continued")
    tk._assert_equal(_np(b.tree_search(2, 2, SEED + 3, node_cap=kcap, trace=True)), plain, "plain", tk.PLAIN)
    assert plain["info"][:, 0].min() == 4
    live = b.fetch("nlegal").cpu().numpy() > 0
    assert (dev["info"][live, 3] & KEPT).all() and (dev_g["info"][live[2:5], 3] & KEPT).all()
    assert (dev["kept"][2:5, 0] != dev_g["kept"][:, 0]).any()          # two different trees of the same rows
    g0 = b.tree_open(1, 1, None, cap, group=0, keep=True, played=act[0:2].contiguous())
    assert not g0.cpu().numpy().any()                                  # group 0 had none


# ---- 10. groups on streams -----------------------------------------------------------------------------------------------------------
def test_two_groups_on_two_streams_equal_the_sessions_run_one_after_the_other():
    regs = tk._small_regions()[2:] + tk._small_regions()[2:4]
    kw = dict(device=DEV, auto_reset=False)
    a, t = RegionBatch(regs, **kw), RegionBatch(regs, **kw)
    for x in (a, t):
        x.set_groups([0, 2, 5])
        x.reset()
    K = a.k_max
    cap = 1 + 4 * 7 * K
    torch.cuda.synchronize()
    cur = torch.cuda.current_stream()
    streams = [torch.cuda.Stream() for _ in range(2)]
    plies = 3
    results = {0: [], 1: []}
    state = {g: dict(played=None) for g in (0, 1)}
    for ply in range(plies):                                     # interleaved: ply by ply, wave by wave, each group on its own stream
        for g, s in enumerate(streams):
            s.wait_stream(cur)
            with torch.cuda.stream(s):
                state[g]["kept"] = a.tree_open(3, 6, None, cap, group=g, stream=s, keep=True, played=state[g]["played"])
        for w in range(2):
            lv = {}
            for g, s in enumerate(streams):
                with torch.cuda.stream(s):
                    lv[g] = a.tree_leaves(group=g, stream=s)
            for g, s in ((1, streams[1]), (0, streams[0])):
                with torch.cuda.stream(s):
                    value, prior = _synthetic(lv[g], K, True)
                    state[g]["res"] = a.tree_backup(value, prior, group=g, stream=s)
        for g, s in enumerate(streams):
            with torch.cuda.stream(s):
                act = XRouteVectorEnv._most_visited(state[g]["res"])
                a.step_group(g, act, stream=s)
                results[g].append(dict(state[g]["res"], kept=state[g]["kept"]))
                state[g]["played"] = act
    for s in streams:
        cur.wait_stream(s)
    torch.cuda.synchronize()
    for g in range(2):
        pair, played = Pair(t, group=g), None
        for ply in range(plies):
            dev, _ = pair.run(played, 2, 3, cap, ("one after the other", g, ply), leaf_priors=True)
            got = _np(results[g][ply])
            for k in RESULT + ("kept",):
                _same(got[k], dev[k], (g, ply, k))
            played = _act(dev)
            t.step_group(g, played)
        assert (dev["info"][:, 3] & KEPT).any()


# ---- 11. refusals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(force_scratch_field=True), dict(stream_per_region=True)])
def test_reopen_refuses_the_scratch_forms_by_name(kw):
    regions = [generate_region(3000 + i, dims=(12, 10, 4), k_range=(3, 6)) for i in range(4)]
    b = RegionBatch(regions, device=DEV, **kw)
    b.reset()
    before = _snapshot(b)
    with pytest.raises(_lib.XRouteError) as ei:
        b.tree_open(2, 4, keep=True)
    assert ei.value.code == _lib.XR_ERR_RANGE and "xr_batch_tree_reopen" in str(ei.value)
    with pytest.raises(_lib.XRouteError) as ei:
        b.tree_leaves()                                          # no session came of it
    assert ei.value.code == _lib.XR_ERR_STATE
    assert _snapshot(b) == before
    b.step(b.random_actions(SEED))            # still usable


# ---- 12. the vector env and whole episodes ---------------------------------------------------------------------------------------------
def test_vector_env_reopen_whole_batch_and_group():
    regions = tk._small_regions()[2:] + tk._small_regions()[2:4]
    env = XRouteVectorEnv(regions, n_envs=5, device=DEV, groups=[0, 2, 5], with_observation=False)
    env.reset()
    b = env.batch
    K = b.k_max
    cap = 1 + 4 * 7 * K

    def session(group, played):
        kept = env.tree_open(3, 6, None, cap, group=group, keep=True, played=played)
        for _ in range(2):
            lv = env.tree_leaves(group=group)
            if group is not None:
                env.step_wait(group)          # (the evaluator below runs on the current stream: it waits for the group's leaves)
            value, prior = _synthetic(lv, K, True)
            res = env.tree_backup(value, prior, group=group)
        if group is not None:
            env.step_wait(group)
        return _np(dict(res, kept=kept))

    whole = session(None, None)
    part = session(1, None)
    for k in RESULT:
        _same(part[k], whole[k][2:5], k)
    act = _act(whole)
    torch.cuda.synchronize()
    b.step(act)
    whole2 = session(None, act)
    part2 = session(1, act[2:5].contiguous())
    torch.cuda.synchronize()
    for k in RESULT + ("kept",):
        _same(part2[k], whole2[k][2:5], k)
    assert (whole2["info"][:, 3] & KEPT).all() and (whole2["kept"][:, 0] > 0).all()
    with pytest.raises(ValueError, match="played"):
        env.tree_open(3, 6, played=act)


def test_evaluated_episodes_with_reuse_end_every_region_and_replay_on_the_oracle():
    from oracle import xr_oracle as orc
    from xroute_env_amd.agents import ActorCritic
    from xroute_env_amd.envs.tree_eval import critic_evaluator, evaluated_episodes
    regions = te._pack(slice(5, 200, 13))[:4]
    torch.manual_seed(7)
    model = ActorCritic(device=DEV).to(DEV).eval()
    stats = {}
    out = evaluated_episodes(regions, critic_evaluator(model), 3, 4, device=DEV, stats=stats, reuse=True, waves_after=2)
    assert len(out) == 4 and stats["routed_nets"] > 0 and stats["plies"] == sum(r.n_nets for r in regions)
    assert stats["carried_visits"] > 0 and stats["carried_nodes"] > 0
    for r, o in zip(regions, out):
        env = orc.OracleEnv(r)
        env.reset()
        nets = sorted(int(v) for v in env.legal())
        assert sorted(o["order"]) == nets and sorted(o["best_order"]) == nets          # permutations of the region's nets
        tot = 0.0
        for a in o["order"]:
            ref = env.step(a)
            assert not ref["status"] & te.BAD
            tot = tot + orc.reward(*[int(v) for v in ref["delta"]])
        assert env.nlegal() == 0 and tot == o["ret"]                                  # every region ends done
        assert o["best_ret"] >= o["ret"] and o["simulations"] == 12 + 8 * (len(o["order"]) - 1)
