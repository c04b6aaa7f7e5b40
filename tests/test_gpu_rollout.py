"""Rollouts on the MI355X (xr_batch_rollout / RegionBatch.rollout / XRouteVectorEnv.rollout, rollout_actions): every env's episode played
to its end from the current state, R times, without stepping.  Twin equivalence (rollout r == a twin batch stepped to the end with
random_actions(rollout_seed(seed, r)), bit for bit); oracle parity for EVERY (env, rollout); slot reuse; prefixes; max_plies; purity;
every router variant; refusals; done envs; env groups on their own streams; several legal words; 4096 ispd18_test1 slots; the vector
env's best-of-R policy."""
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
SEED = 0x5011
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAD = _lib.XR_ENV_BAD_ACTION
M64 = 2 ** 64 - 1


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
    """Regions of different sizes, one with N % 8 != 0 (13 x 17 x 4: the tail of the vector copy of the owner row)."""
    from tests.helpers import obs_set_regions
    extra = [generate_region(9100 + i, dims=d, k_range=(4, 10), pins=(3, 5), net_span=7)
             for i, d in enumerate([(16, 12, 5), (20, 14, 6), (13, 17, 4), (24, 20, 5)])]
    return obs_set_regions("mixed") + extra


def _snapshot(b):
    """Every array xr_batch_fetch returns, as bytes."""
    return {k: b.fetch(k).cpu().numpy().tobytes() for k in b._FETCH}


def _legal_matrix(b):
    """bool [n_envs, k_max]: net n (column n - 1) is legal."""
    words = b.fetch("legal").cpu().numpy().view(np.uint64)
    bits = ((words[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).astype(bool)
    return bits.reshape(words.shape[0], -1)[:, :max(b.k_max, 1)]


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _advance(b, steps, history=None, start=0):
    """Random steps number start .. start + steps - 1 (the seed of a step is its number's); history[e] collects the nets env e routed."""
    for i in range(start, start + steps):
        act = b.random_actions(SEED + 1000 + i)
        b.step(act)
        if history is not None:
            for e, a in enumerate(act.cpu().numpy().tolist()):
                if a:
                    history[e].append(a)


def _play_to_the_end(t, seed_r, k_most):
    """Step batch `t` (auto_reset off) to the end with random_actions(seed_r).  What a rollout must equal: per env the order, the summed
    deltas, the status OR, the plies, the path-length sum, the final hash and nlegal, the rewards summed in step order from 0.0."""
    n = t.n_envs
    cum0 = t.fetch("cum").cpu().numpy().copy()
    order = np.zeros((n, max(t.k_max, 1)), np.int32)
    status, plies, plen = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    ret = np.zeros(n, np.float64)
    act = torch.empty(n, dtype=torch.int32, device=DEV)
    for _ in range(k_most + 1):
        a = t.random_actions(seed_r, act).cpu().numpy()
        live = np.flatnonzero(a > 0)
        if live.size == 0:
            break
        t.step(act)
        rec = t.records()
        assert not (rec["status"][live] & BAD).any()
        order[live, plies[live]] = a[live]
        plies[live] += 1
        status[live] |= rec["status"][live].astype(np.int32)
        plen[live] += rec["path_len"][live]
        ret[live] = ret[live] + rec["reward"][live]
    else:
        raise AssertionError("the twin did not finish")
    return dict(order=order, delta=t.fetch("cum").cpu().numpy() - cum0, status=status, plies=plies, plen=plen, ret=ret,
                hash=t.fetch("hash").cpu().numpy(), nlegal=t.fetch("nlegal").cpu().numpy())


def _assert_equals_twin(res, r, tw, what):
    out = res["out"][:, r]
    assert np.array_equal(res["order"][:, r], tw["order"]), (what, "order")
    assert np.array_equal(out[:, :3], tw["delta"]), (what, "delta")
    assert np.array_equal(out[:, 3], tw["status"]), (what, "status")
    assert np.array_equal(out[:, 4], tw["plies"]), (what, "plies")
    assert np.array_equal(out[:, 5], tw["nlegal"]) and (out[:, 5] == 0).all(), (what, "nlegal_end")
    assert np.array_equal(out[:, 6], tw["plen"]), (what, "path_len_sum")
    assert (out[:, 7] == 0).all(), what
    assert np.array_equal(res["hash"][:, r], tw["hash"]), (what, "hash")
    assert np.array_equal(res["ret"][:, r].view(np.uint64), tw["ret"].view(np.uint64)), (what, "return bits")


def _twin_equivalence(regions, kw, n, R, states, k_most):
    """Rollouts of `a` at the listed step counts against fresh twins brought to the same state."""
    a = RegionBatch(regions, n_envs=n, device=DEV, **kw)
    a.reset()
    taken = 0
    compared = 0
    for at in states:
        _advance(a, at - taken, start=taken)
        taken = at
        res = _np(a.rollout(R, SEED))
        for r in range(R):
            t = RegionBatch(regions, n_envs=n, device=DEV, **kw)
            t.reset()
            _advance(t, at)
            assert t.fetch("hash").cpu().numpy().tobytes() == a.fetch("hash").cpu().numpy().tobytes()
            _assert_equals_twin(res, r, _play_to_the_end(t, _lib.rollout_seed(SEED, r), k_most), (at, r))
            compared += n
            t.close()
    return compared


def _oracle_check(regions, reg, history, res, okw=None, order=None, what=""):
    """Replay every order on the oracle after the env's history: delta totals, status OR, plies, nlegal_end, hash and the return bits of
    EVERY (env, rollout).  order: the nets to replay (default: the rollout's own order_out).  Returns the number compared."""
    from oracle import xr_oracle as orc
    out, ret, hsh = res["out"], res["ret"], res["hash"].view(np.uint64)
    order = res["order"] if order is None else order
    compared = 0
    for e in range(out.shape[0]):
        for r in range(out.shape[1]):
            env = orc.OracleEnv(regions[int(reg[e])], **(okw or {}))
            env.reset()
            for a in history[e]:
                env.step(a)
            c0 = env.cum()
            st, tot, plies = 0, 0.0, int(out[e, r, 4])
            nets = [int(v) for v in order[e, r] if v > 0]
            assert len(nets) == plies and (res["order"][e, r, plies:] == 0).all(), (what, e, r, nets, plies)
            assert res["order"][e, r, :plies].tolist() == nets, (what, e, r)
            for a in nets:
                ref = env.step(a)
                assert not ref["status"] & BAD, (what, e, r, a)
                st |= ref["status"]
                tot = tot + orc.reward(*[int(v) for v in ref["delta"]])
            assert out[e, r, :3].tolist() == (env.cum() - c0).tolist(), (what, e, r, out[e, r], env.cum() - c0)
            assert int(out[e, r, 3]) & ~BAD == st, (what, e, r, out[e, r, 3], st)
            assert int(out[e, r, 5]) == env.nlegal() and int(out[e, r, 7]) == 0, (what, e, r)
            assert int(hsh[e, r]) == env.hash() & M64, (what, e, r)
            assert ret[e, r:r + 1].view(np.uint64)[0] == np.array([tot]).view(np.uint64)[0], (what, e, r, ret[e, r], tot)
            compared += 1
    return compared


def _batch_with_history(regions, n, steps, **kw):
    b = RegionBatch(regions, n_envs=n, device=DEV, **kw)
    b.reset()
    history = [[] for _ in range(n)]
    _advance(b, steps, history)
    return b, history, b.fetch("region").cpu().numpy()


# ---- 1. twin equivalence ---------------------------------------------------------------------------------------------------------
def test_every_rollout_equals_a_twin_batch_stepped_to_the_end_with_its_seed():
    regions = _mixed_regions()
    compared = _twin_equivalence(regions, {}, 24, 3, (0, 2, 5), max(r.n_nets for r in regions))
    assert compared == 3 * 3 * 24


# ---- 2. oracle parity, nothing left out ------------------------------------------------------------------------------------------
def test_every_rollout_equals_the_oracle_replay_of_its_order():
    regions = _mixed_regions()
    n, R = 24, 3
    b = RegionBatch(regions, n_envs=n, device=DEV)
    b.reset()
    reg = b.fetch("region").cpu().numpy()
    history = [[] for _ in range(n)]
    compared = taken = 0
    for at in (0, 2, 5):
        _advance(b, at - taken, history, start=taken)
        taken = at
        nl = b.fetch("nlegal").cpu().numpy()
        res = _np(b.rollout(R, SEED + at))
        assert np.array_equal(res["out"][:, :, 4], np.repeat(nl[:, None], R, 1))          # random to the end: every legal net routed
        compared += _oracle_check(regions, reg, history, res, what=at)
    assert compared == 3 * n * R


# ---- 3. slot reuse ---------------------------------------------------------------------------------------------------------------
def test_more_tasks_than_resident_workgroups_reuse_the_shadow_slots():
    regions = _mixed_regions()
    n, R = 24, 64
    b, history, reg = _batch_with_history(regions, n, 2)
    legal = _legal_matrix(b)
    res = _np(b.rollout(R, SEED))
    assert res["out"].shape == (n, R, 8)
    assert _oracle_check(regions, reg, history, res) == n * R == 1536
    for e in range(n):
        want = (np.flatnonzero(legal[e]) + 1).tolist()
        for r in range(R):
            assert sorted(v for v in res["order"][e, r].tolist() if v) == want, (e, r)
    assert any(len({tuple(o) for o in res["order"][e].tolist()}) > 1 for e in range(n))          # the seeds differ


# ---- 4. prefix -------------------------------------------------------------------------------------------------------------------
def test_full_explicit_orders_with_stop_equal_the_oracle_replay():
    regions = _mixed_regions()
    n, R = 24, 2
    b, history, reg = _batch_with_history(regions, n, 2)
    legal = _legal_matrix(b)
    rng = np.random.default_rng(5)
    prefix = np.zeros((n, R, b.k_max + 1), np.int32)
    for e in range(n):
        for r in range(R):
            nets = rng.permutation(np.flatnonzero(legal[e]) + 1)
            prefix[e, r, :nets.size] = nets
    before = _snapshot(b)
    res = _np(b.rollout(R, SEED, policy="stop", prefix=torch.from_numpy(prefix).to(DEV)))
    assert _snapshot(b) == before
    assert np.array_equal(res["order"], prefix[:, :, :b.k_max])
    assert (res["out"][:, :, 3] & BAD == 0).all() and (res["out"][:, :, 5] == 0).all()
    assert _oracle_check(regions, reg, history, res, order=prefix) == n * R


def test_prefix_entries_that_are_not_legal_are_skipped_flagged_and_cost_no_ply():
    regions = _mixed_regions()
    n = 24
    b, history, reg = _batch_with_history(regions, n, 2)
    legal = _legal_matrix(b)
    prefix = np.zeros((n, 3, 8), np.int32)
    real = np.zeros((n, 3, 8), np.int32)
    flagged = np.zeros((n, 3), bool)
    for e in range(n):
        nets = (np.flatnonzero(legal[e]) + 1).tolist()
        if not nets:                                                   # a done env: the empty rollout, nothing looked at, nothing flagged
            prefix[e, :, :2] = [history[e][0], 1]
            continue
        a, c = nets[0], nets[-1]
        prefix[e, 0, :4] = [a, a, c, a]                                # repeated
        real[e, 0, :2] = [a, c] if c != a else [a, 0]
        prefix[e, 1, :5] = [history[e][0], a, b.k_max + 7, 70000, c]   # already routed, beyond k_max, beyond every legal word
        real[e, 1, :2] = real[e, 0, :2]
        prefix[e, 2, :3] = [c, 0, a]                                   # the terminator ends the list: `a` is never seen
        real[e, 2, :1] = [c]
        flagged[e] = [True, True, False]
        if len(nets) == 1:                                             # (everything routed after the first: the rest of a list is ignored)
            flagged[e, 0] = False
            flagged[e, 1] = True                                       # (the already-routed net comes first)
    res = _np(b.rollout(3, SEED, policy="stop", prefix=torch.from_numpy(prefix).to(DEV)))
    assert np.array_equal((res["out"][:, :, 3] & BAD) != 0, flagged)
    assert np.array_equal(res["out"][:, :, 4], (real > 0).sum(2))      # plies: real routes only
    assert np.array_equal(res["order"][:, :, :2], real[:, :, :2]) and not res["order"][:, :, 2:].any()
    assert flagged[:, 0].sum() > 12
    assert _oracle_check(regions, reg, history, res, order=real) == n * 3


def test_a_prefix_of_one_legal_net_with_stop_equals_that_nets_lookahead_entry():
    regions = _mixed_regions()
    n = 24
    b, _, _ = _batch_with_history(regions, n, 2)
    K = b.k_max
    legal = _legal_matrix(b)
    nl = b.fetch("nlegal").cpu().numpy()
    ds, rw = (v.cpu().numpy() for v in b.lookahead())
    prefix = np.zeros((n, K, 1), np.int32)
    for e in range(n):
        nets = np.flatnonzero(legal[e]) + 1
        prefix[e, :nets.size, 0] = nets                                 # one candidate per r; r beyond the env's nets left empty
    res = _np(b.rollout(K, SEED, policy="stop", prefix=torch.from_numpy(prefix).to(DEV)))
    hash0 = b.fetch("hash").cpu().numpy()
    compared = 0
    for e in range(n):
        for r in range(K):
            net = int(prefix[e, r, 0])
            o = res["out"][e, r]
            if net == 0:                                                # nothing to route: the empty rollout of a live env
                assert o.tolist() == [0, 0, 0, 0, 0, int(nl[e]), 0, 0] and res["ret"][e, r:r + 1].view(np.uint64)[0] == 0
                assert res["hash"][e, r] == hash0[e] and not res["order"][e, r].any()
                continue
            assert o[:4].tolist() == ds[e, net - 1].tolist() and o[4] == 1 and o[5] == nl[e] - 1, (e, net)
            want = np.float64(0.0) + rw[e, net - 1:net]                 # (the return is a sum that starts at 0.0)
            assert res["ret"][e, r:r + 1].view(np.uint64)[0] == want.view(np.uint64)[0], (e, net)
            assert res["order"][e, r].tolist() == [net] + [0] * (K - 1)
            compared += 1
    assert compared == int(nl.sum()) > 40


def test_random_continues_from_the_state_the_prefix_left():
    regions = _mixed_regions()
    n, R = 24, 3
    b, history, reg = _batch_with_history(regions, n, 2)
    legal = _legal_matrix(b)
    nl = b.fetch("nlegal").cpu().numpy()
    prefix = np.zeros((n, R, 2), np.int32)
    for e in range(n):
        nets = np.flatnonzero(legal[e]) + 1
        for r in range(R if nets.size else 0):
            two = nets[::-1][r % nets.size:][:2]
            prefix[e, r, :two.size] = two
    res = _np(b.rollout(R, SEED, prefix=torch.from_numpy(prefix).to(DEV)))
    k = (prefix > 0).sum(2)
    for e in range(n):
        for r in range(R):
            assert res["order"][e, r, :k[e, r]].tolist() == prefix[e, r, :k[e, r]].tolist()
    assert np.array_equal(res["out"][:, :, 4], np.repeat(nl[:, None], R, 1)) and (res["out"][:, :, 3] & BAD == 0).all()
    assert _oracle_check(regions, reg, history, res) == n * R
    # the tail is the random policy's: a twin that routes the prefix and then follows random_actions(seed_r) ends the same
    for r in range(R):
        t = RegionBatch(regions, n_envs=n, device=DEV)
        t.reset()
        _advance(t, 2)
        for j in range(2):
            t.step(torch.from_numpy(np.ascontiguousarray(prefix[:, r, j])).to(DEV))
        tw = _play_to_the_end(t, _lib.rollout_seed(SEED, r), b.k_max)
        assert np.array_equal(res["hash"][:, r], tw["hash"]), r
        for e in range(n):
            assert res["order"][e, r, k[e, r]:k[e, r] + tw["plies"][e]].tolist() == tw["order"][e, :tw["plies"][e]].tolist(), (e, r)
        t.close()


# ---- 5. max_plies ----------------------------------------------------------------------------------------------------------------
def test_max_plies_truncates_the_same_rollout():
    regions = _mixed_regions()
    n, R = 24, 2
    b, history, reg = _batch_with_history(regions, n, 2)
    nl = b.fetch("nlegal").cpu().numpy()
    full = _np(b.rollout(R, SEED))
    for cap in (1, 3):
        cut = _np(b.rollout(R, SEED, max_plies=cap))
        plies = np.minimum(nl, cap)
        assert np.array_equal(cut["out"][:, :, 4], np.repeat(plies[:, None], R, 1))
        assert np.array_equal(cut["out"][:, :, 5], np.repeat((nl - plies)[:, None], R, 1))
        assert np.array_equal(cut["order"][:, :, :cap], full["order"][:, :, :cap]) and not cut["order"][:, :, cap:].any()
        assert _oracle_check(regions, reg, history, cut, what=cap) == n * R
    # the prefix's routes count: two prefix nets under max_plies = 2 leave nothing to the policy
    legal = _legal_matrix(b)
    prefix = np.zeros((n, 1, 3), np.int32)
    for e in range(n):
        nets = np.flatnonzero(legal[e]) + 1
        prefix[e, 0, :min(3, nets.size)] = nets[:3]
    cut = _np(b.rollout(1, SEED, prefix=torch.from_numpy(prefix).to(DEV), max_plies=2))
    assert np.array_equal(cut["out"][:, 0, 4], np.minimum(nl, 2))
    assert np.array_equal(cut["order"][:, 0, :2], prefix[:, 0, :2]) and not cut["order"][:, 0, 2:].any()


# ---- 6. purity -------------------------------------------------------------------------------------------------------------------
def test_rollout_leaves_every_fetchable_array_byte_identical():
    regions = _mixed_regions()
    b = RegionBatch(regions, n_envs=24, device=DEV, auto_reset=True, max_route_count=1)
    b.reset()
    act = torch.empty(24, dtype=torch.int32, device=DEV)
    for step in range(12):
        before = _snapshot(b)
        b.rollout(2, SEED + step)
        if step % 3 == 0:
            b.rollout(1, SEED, policy="stop", prefix=torch.full((24, 1, 2), 1 + step, dtype=torch.int32, device=DEV))
            b.rollout(3, SEED, max_plies=2)
        after = _snapshot(b)
        for k in before:
            assert before[k] == after[k], (step, k)
        b.step(b.random_actions(SEED + step, act))


@pytest.mark.parametrize("mode", ["route", "inplace", "inplace_u8"])
def test_a_batch_that_rolls_out_before_every_step_equals_its_twin_that_never_does(mode):
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
    for step in range(50):
        res = a.rollout(2, SEED + step)
        a.random_actions(_lib.rollout_seed(SEED + step, 1), act)
        assert torch.equal(res["order"][:, 1, 0], act), step             # the first ply of rollout 1 is the action this seed takes now
        a.step(act, obs_a, inplace=True) if obs_a is not None else a.step(act)
        t.step(act, obs_t, inplace=True) if obs_t is not None else t.step(act)
        for k in ("hash", "record", "owner", "legal", "region", "replay", "env_steps", "steps", "path", "path_len", "sweeps"):
            assert a.fetch(k).cpu().numpy().tobytes() == t.fetch(k).cpu().numpy().tobytes(), (step, k)
        if obs_a is not None:
            info = a.observe_info()
            assert info["form"] == 3 and info["inplace"], (step, info)          # the in-place path survived the rollout
            assert torch.equal(obs_a, obs_t), step


# ---- 7. variants -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["auto", "sweep", "dial", "dial_r2", "v2_guides"])
def test_rollout_under_every_router_variant(variant):
    if variant == "v2_guides":
        regions = _pack(slice(5, 200, 13))[:12]
        assert all(r.guide_off is not None and r.guide_off[-1] > 0 for r in regions)
        kw = dict(guide_cost=1000, guide_margin=1, maze_end_iter=3)
    else:
        regions = [generate_region(3000 + i) for i in range(12)]
        kw = dict(router={"auto": 0, "sweep": 1, "dial": 2, "dial_r2": 3}[variant], dial_mult=0 if variant != "dial" else 5)
    n = 2 * len(regions)
    assert _twin_equivalence(regions, kw, n, 2, (0, 3), max(r.n_nets for r in regions)) == 2 * 2 * n


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(force_scratch_field=True), dict(stream_per_region=True)])
def test_rollout_refuses_the_scratch_forms_and_leaves_the_batch_untouched(kw):
    regions = [generate_region(3000 + i, dims=(12, 10, 4), k_range=(3, 6)) for i in range(4)]
    b = RegionBatch(regions, device=DEV, **kw)
    b.reset()
    b.step(b.random_actions(SEED))
    before = _snapshot(b)
    with pytest.raises(_lib.XRouteError) as ei:
        b.rollout(2, SEED)
    assert ei.value.code == _lib.XR_ERR_RANGE
    assert _snapshot(b) == before
    b.step(b.random_actions(SEED + 1))            # still usable


def test_rollout_argument_errors_on_a_live_batch():
    regions = [generate_region(3000 + i, dims=(12, 10, 4), k_range=(3, 6)) for i in range(4)]
    b = RegionBatch(regions, device=DEV)
    b.reset()
    b.step(b.random_actions(SEED))
    K = b.k_max
    out = torch.empty((4, 2, 8), dtype=torch.int32, device=DEV)
    order = torch.empty((4, 2, K), dtype=torch.int32, device=DEV)
    prefix = torch.zeros((4, 2, 2), dtype=torch.int32, device=DEV)
    p, po, pp = (C.c_void_p(t.data_ptr()) for t in (out, order, prefix))
    before = _snapshot(b)
    L = b.L

    def call(group=-1, R=2, policy=1, prefix=None, stride=0, max_plies=0, out=p, order=None, k_cap=0):
        return L.xr_batch_rollout(b._h, group, R, policy, 7, prefix, stride, max_plies, out, None, None, order, k_cap, None)

    for kw, code, word in ((dict(out=None), _lib.XR_ERR_INVALID, b"null"), (dict(group=1), _lib.XR_ERR_INVALID, b"group"),
                           (dict(group=-2), _lib.XR_ERR_INVALID, b"group"), (dict(policy=2), _lib.XR_ERR_INVALID, b"policy"),
                           (dict(policy=-1), _lib.XR_ERR_INVALID, b"policy"), (dict(prefix=pp, stride=0), _lib.XR_ERR_INVALID, b"prefix_stride"),
                           (dict(prefix=pp, stride=-2), _lib.XR_ERR_INVALID, b"prefix_stride"), (dict(max_plies=-1), _lib.XR_ERR_INVALID, b"max_plies"),
                           (dict(R=0), _lib.XR_ERR_RANGE, b"n_rollouts"), (dict(R=_lib.XR_ROLLOUT_MAX + 1), _lib.XR_ERR_RANGE, b"n_rollouts"),
                           (dict(order=po, k_cap=K - 1), _lib.XR_ERR_RANGE, b"k_cap")):
        assert call(**kw) == code, kw
        msg = L.xr_last_error()
        assert b"xr_batch_rollout" in msg and word in msg, (kw, msg)
    assert _snapshot(b) == before
    with pytest.raises(ValueError):
        b.rollout(2, out=out.to(torch.int64))
    with pytest.raises(ValueError):
        b.rollout(2, prefix=prefix.to(torch.int64))
    # the optional outputs may be null, k_cap is ignored without order_out, a wider k_cap pads the order rows with 0
    assert call(k_cap=-3) == 0
    wide = torch.full((4, 2, K + 3), 77, dtype=torch.int32, device=DEV)
    assert call(order=C.c_void_p(wide.data_ptr()), k_cap=K + 3) == 0
    res = b.rollout(2, 7)
    assert torch.equal(res["out"], out) and torch.equal(wide[:, :, :K], res["order"]) and not wide[:, :, K:].any()
    assert _snapshot(b) == before
    b.step(b.random_actions(SEED + 1))            # still usable


# ---- 9. done envs and auto-reset -------------------------------------------------------------------------------------------------
def test_done_envs_of_an_auto_reset_batch_hold_the_empty_rollout():
    regions = _mixed_regions()
    n, R = 24, 2
    b = RegionBatch(regions, n_envs=n, device=DEV, auto_reset=True, max_route_count=1)
    b.reset()
    act = torch.empty(n, dtype=torch.int32, device=DEV)
    done_seen = live_seen = 0
    for step in range(12):
        nl = b.fetch("nlegal").cpu().numpy()
        h = b.fetch("hash").cpu().numpy()
        res = _np(b.rollout(R, SEED + step))
        done = nl == 0
        assert not res["out"][done].any() and not res["order"][done].any()
        assert (res["ret"][done].view(np.uint64) == 0).all()                       # +0.0
        assert np.array_equal(res["hash"][done], np.repeat(h[done, None], R, 1))
        assert np.array_equal(res["out"][~done][:, :, 4], np.repeat(nl[~done, None], R, 1))
        assert (res["out"][:, :, 3] & _lib.XR_ENV_WAS_RESET == 0).all()            # never through an auto-reset
        done_seen += int(done.sum()); live_seen += int((~done).sum())
        b.step(b.random_actions(SEED + step, act))
    assert done_seen > 0 and live_seen > 0


# ---- 10. groups ------------------------------------------------------------------------------------------------------------------
def test_groups_roll_out_on_their_own_streams_between_steps_of_other_groups():
    regions = [generate_region(3000 + i) for i in range(8)] + _mixed_regions()[:6]
    n, R = 40, 2
    kw = dict(n_envs=n, device=DEV, auto_reset=True, max_route_count=1)
    a, t = RegionBatch(regions, **kw), RegionBatch(regions, **kw)
    a.set_groups(4)
    a.reset(); t.reset()
    torch.cuda.synchronize()
    cur = torch.cuda.current_stream()
    streams = [torch.cuda.Stream() for _ in range(4)]
    cadence = [1, 2, 3, 2]
    rounds = 4
    results = {g: [] for g in range(4)}
    for s in streams:
        s.wait_stream(cur)
    for r in range(rounds):
        for k in range(max(cadence)):
            for g in range(4):
                if k >= cadence[g]:
                    continue
                s = streams[g]
                with torch.cuda.stream(s):
                    results[g].append(a.rollout(R, SEED, group=g, stream=s))          # count = steps taken so far by this group
                    act = a.random_actions_group(g, SEED, stream=s)
                    a.step_group(g, act, stream=s)
    for s in streams:
        cur.wait_stream(s)
    torch.cuda.synchronize()
    # lock-step twin: whole-batch rollout before every step
    twin = []
    act = torch.empty(n, dtype=torch.int32, device=DEV)
    for i in range(rounds * max(cadence)):
        twin.append(_np(t.rollout(R, SEED)))
        t.step(t.random_actions(SEED, act))
    for g in range(4):
        lo, hi = a.group_bounds(g)
        assert len(results[g]) == rounds * cadence[g]
        for i, res in enumerate(results[g]):
            res = _np(res)
            assert res["out"].shape == (hi - lo, R, 8)
            for k in ("out", "hash", "order"):
                assert np.array_equal(res[k], twin[i][k][lo:hi]), (g, i, k)
            assert np.array_equal(res["ret"].view(np.uint64), twin[i]["ret"][lo:hi].view(np.uint64)), (g, i)


# ---- 11. many nets ---------------------------------------------------------------------------------------------------------------
def test_a_region_with_several_legal_words_rolls_out_every_net():
    from tests.helpers import OBS_MANY_NETS
    regions = [generate_region(9300, **OBS_MANY_NETS)]
    b = RegionBatch(regions, n_envs=1, device=DEV)
    assert b.legal_words >= 4
    b.reset()
    legal = _legal_matrix(b)
    nets = (np.flatnonzero(legal[0]) + 1).tolist()
    assert len(nets) > 128 and max(nets) > 192                                   # legal nets in the fourth word
    res = _np(b.rollout(2, SEED))
    for r in range(2):
        assert sorted(v for v in res["order"][0, r].tolist() if v) == nets, r
    assert res["order"][0, 0].tolist() != res["order"][0, 1].tolist()
    assert (res["out"][0, :, 4] == len(nets)).all() and (res["out"][0, :, 5] == 0).all()
    assert _oracle_check(regions, [0], [[]], res) == 2


# ---- 12. full size ---------------------------------------------------------------------------------------------------------------
def test_rollouts_at_4096_ispd18_slots_equal_what_the_batch_then_does():
    b = RegionBatch(_pack(), n_envs=4096, device=DEV, auto_reset=False)
    b.reset()
    _advance(b, 3)
    res = b.rollout(2, SEED)
    first = b.random_actions(_lib.rollout_seed(SEED, 0))
    assert torch.equal(res["order"][:, 0, 0], first)
    res = _np(res)
    tw = _play_to_the_end(b, _lib.rollout_seed(SEED, 1), b.k_max)
    _assert_equals_twin(res, 1, tw, "4096 slots")
    assert tw["plies"].sum() > 4096


# ---- 13. vector env --------------------------------------------------------------------------------------------------------------
def test_vector_env_rollout_actions_and_an_episode_driven_by_them():
    from xroute_env_amd.envs.vector_env import XRouteVectorEnv
    regions = _mixed_regions()
    env = XRouteVectorEnv(regions, n_envs=24, device=DEV, max_route_count=1)
    env.reset()
    k_most = max(r.n_nets for r in regions)
    finished = np.zeros(24, bool)
    for step in range(k_most + 2):
        res = _np(env.rollout(4, SEED + step))
        act = env.rollout_actions(4, SEED + step)
        want = res["order"][np.arange(24), np.argmax(res["ret"], axis=1), 0]          # (np.argmax: the first maximum)
        assert act.dtype == torch.int32 and np.array_equal(act.cpu().numpy(), want), step
        nl = env.batch.fetch("nlegal").cpu().numpy()
        assert np.array_equal(act.cpu().numpy() == 0, nl == 0)
        _, _, done, info = env.step(act)
        rec = env.batch.records()
        live = nl > 0
        assert not (rec["status"][live] & BAD).any(), step
        finished |= done.cpu().numpy().astype(bool)
    assert finished.all()


def test_vector_env_group_rollout_actions_equal_the_whole_batch_rows():
    from xroute_env_amd.envs.vector_env import XRouteVectorEnv
    regions = _mixed_regions()
    env = XRouteVectorEnv(regions, n_envs=24, device=DEV, max_route_count=1, groups=3, with_observation=False)
    env.reset()
    whole = env.rollout_actions(3, SEED).cpu().numpy()
    whole_res = _np(env.rollout(3, SEED))
    for g in range(3):
        lo, hi = env.batch.group_bounds(g)
        res = env.rollout(3, SEED, group=g)
        act = env.rollout_actions(3, SEED, g)
        env.step_wait(g)
        assert np.array_equal(act.cpu().numpy(), whole[lo:hi])
        assert np.array_equal(res["out"].cpu().numpy(), whole_res["out"][lo:hi])
        env.step_async(act, g)
    env.step_wait()
    torch.cuda.synchronize()
