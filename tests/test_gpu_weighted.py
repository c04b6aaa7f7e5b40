"""Weighted net sampling on the MI355X (XR-Pick v1: xr_batch_weighted_actions, xr_batch_rollout_weighted, xr_batch_tree_search_weighted,
envs.weighted.cem_search).  Unit weights are the random policy bit for bit; the device pick against the spec's twin in Python integers
(tests/weighted_twin.py) on regions of 1, 64, 65-70 and 200+ nets; every weighted rollout equals a twin batch stepped to the end with
weighted_actions(weights, rollout_seed(seed, r)) and the oracle's replay of its order; zero-weight nets come last; purity; refusals; env
groups on their own streams; every router variant; the weighted tree search against tests/tree_twin.py; CEM; 4096 ispd18_test1 slots."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from tests import tree_twin, weighted_twin as wt
from tests.helpers import OBS_MANY_NETS
from tests.test_gpu_rollout import (_advance, _assert_equals_twin, _batch_with_history, _legal_matrix, _mixed_regions, _np, _oracle_check, _pack,
                                    _snapshot)
from xroute_env_amd import _lib
from xroute_env_amd.batch import RegionBatch
from xroute_env_amd.envs.weighted import cem_search
from xroute_env_amd.regions import generate_region

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x3E16
BAD = _lib.XR_ENV_BAD_ACTION
WMAX = _lib.XR_WEIGHT_MAX


@pytest.fixture(autouse=True)
def _release_cached_memory():
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _weights(rows, k, seed, hi=WMAX, zero=0.0):
    """int32 [rows, k] on the device: uniform in [0, hi], a share `zero` of the entries 0."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, hi + 1, size=(rows, k), dtype=np.int64)
    w[rng.random((rows, k)) < zero] = 0
    return torch.from_numpy(w.astype(np.int32)).to(DEV).contiguous()


def _ones(b):
    return torch.ones((b.n_envs, max(b.k_max, 1)), dtype=torch.int32, device=DEV)


def _assert_same_rollouts(a, b, what):
    for k in ("out", "hash", "order"):
        assert np.array_equal(a[k], b[k]), (what, k)
    assert np.array_equal(a["ret"].view(np.uint64), b["ret"].view(np.uint64)), (what, "return bits")


def _play_weighted(t, weights, seed_r, k_most, prefix=None):
    """Step batch `t` (auto_reset off) through the columns of `prefix` (int32 [n, cols]; 0: the env sits the step out), then to the end
    with weighted_actions(weights, seed_r).  What a weighted rollout must equal, as test_gpu_rollout._play_to_the_end lists it."""
    n = t.n_envs
    cum0 = t.fetch("cum").cpu().numpy().copy()
    order = np.zeros((n, max(t.k_max, 1)), np.int32)
    status, plies, plen = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    ret = np.zeros(n, np.float64)
    act = torch.empty(n, dtype=torch.int32, device=DEV)
    cols = [] if prefix is None else [np.ascontiguousarray(prefix[:, j]) for j in range(prefix.shape[1])]
    for i in range(len(cols) + k_most + 1):
        if i < len(cols):
            act.copy_(torch.from_numpy(cols[i]))
            a = cols[i]
        else:
            a = t.weighted_actions(weights, seed_r, act).cpu().numpy()
        live = np.flatnonzero(a > 0)
        if live.size == 0:
            if i < len(cols):
                continue
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


def _twin_pick(b, weights, seed, lo=0):
    """XR-Pick v1 in Python integers for every env of `b`, from the fetched legal words and env_steps."""
    legal = b.fetch("legal").cpu().numpy().view(np.uint64)
    steps = b.fetch("env_steps").cpu().numpy()
    w = weights.cpu().numpy().tolist()
    return np.array([wt.pick(wt.legal_nets(legal[e]), int(steps[e]), e, seed, w[e - lo]) for e in range(lo, lo + len(w))], np.int32)


# ---- 1. unit weights are the random policy ---------------------------------------------------------------------------------------------
def test_unit_weights_are_the_random_policy_bit_for_bit():
    regions = _mixed_regions()
    n, R = 24, 3
    b = RegionBatch(regions, n_envs=n, device=DEV)
    b.reset()
    w = _ones(b)
    taken = 0
    for at in (0, 2, 5):
        _advance(b, at - taken, start=taken)
        taken = at
        for seed in (SEED + at, 2 ** 64 - 1 - at):
            assert torch.equal(b.weighted_actions(w, seed), b.random_actions(seed)), (at, seed)
        _assert_same_rollouts(_np(b.rollout(R, SEED + at, policy="weighted", weights=w)), _np(b.rollout(R, SEED + at, policy="random")), at)
        # ... and so are all weights 0: the fallback
        assert torch.equal(b.weighted_actions(torch.zeros_like(w), SEED), b.random_actions(SEED)), at
    assert (b.fetch("nlegal") > 0).any()


# ---- 2. the pick against the Python twin -----------------------------------------------------------------------------------------------
def _pick_regions(kind):
    many = dict(dims=(23, 15, 5), net_span=6, pins=(2, 2), aps=(1, 1))
    if kind == "one_net":
        return [generate_region(9400 + i, dims=(7, 9, 5), k_range=(1, 1), net_span=4) for i in range(2)]
    if kind == "exactly_64":
        return [generate_region(9410 + i, k_range=(64, 64), blockage=(0.02, 0.04), prerouted=(0.0, 0.01), **many) for i in range(2)]
    if kind == "crosses_a_word":
        return [generate_region(9420 + i, k_range=(65 + 2 * i, 66 + 2 * i), blockage=(0.02, 0.04), prerouted=(0.0, 0.01), **many) for i in range(3)]
    return [generate_region(9300 + i, **OBS_MANY_NETS) for i in range(2)]


@pytest.mark.parametrize("kind", ["one_net", "exactly_64", "crosses_a_word", "four_words"])
def test_the_device_pick_equals_the_twin_in_python_integers(kind):
    regions = _pick_regions(kind)
    n = 6
    b = RegionBatch(regions, n_envs=n, device=DEV)
    b.reset()
    K = b.k_max
    nl0 = b.fetch("nlegal").cpu().numpy()
    want_nl = {"one_net": (1, 1), "exactly_64": (64, 64), "crosses_a_word": (65, 70), "four_words": (193, 255)}[kind]
    assert want_nl[0] <= nl0.min() and nl0.max() <= want_nl[1], nl0          # every declared net has access points
    assert b.legal_words == {"one_net": 1, "exactly_64": 1, "crosses_a_word": 2, "four_words": 4}[kind]
    rng = np.random.default_rng(11)
    one = np.zeros((n, K), np.int32)
    one[np.arange(n), rng.integers(0, K, n)] = 5
    wild = rng.integers(-2 ** 31, 2 ** 31, size=(n, K), dtype=np.int64).astype(np.int32)          # above the clamp and negative
    patterns = {"random": _weights(n, K, 1), "three quarters zero": _weights(n, K, 2, zero=0.75), "all zero": torch.zeros((n, K), dtype=torch.int32, device=DEV),
                "one positive": torch.from_numpy(one).to(DEV), "clamped and negative": torch.from_numpy(wild).to(DEV), "small": _weights(n, K, 3, hi=3)}
    picked, words_hit = 0, set()
    for state in (0, 3):
        _advance(b, state)
        legal = _legal_matrix(b)
        for seed in (SEED, 2 ** 63 + 77):
            for name, w in patterns.items():
                got = b.weighted_actions(w, seed).cpu().numpy()
                want = _twin_pick(b, w, seed)
                assert np.array_equal(got, want), (kind, state, seed, name, got, want)
                live = got > 0
                assert legal[live, got[live] - 1].all()
                picked += int(live.sum())
                words_hit |= set(((got[live] - 1) // 64).tolist())
            # k_cap > k_max: large weights on the nets that are not legal and on columns beyond the region's nets are never read
            wide = np.full((n, K + 7), 2 ** 31 - 1, np.int32)
            base = patterns["small"].cpu().numpy()
            wide[:, :K] = np.where(legal, base, 2 ** 31 - 1)
            wide_t = torch.from_numpy(wide).to(DEV)
            out = torch.empty(n, dtype=torch.int32, device=DEV)
            assert b.L.xr_batch_weighted_actions(b._h, -1, C.c_void_p(wide_t.data_ptr()), K + 7, C.c_void_p(out.data_ptr()), C.c_uint64(seed), None) == 0
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), _twin_pick(b, patterns["small"], seed)), (kind, state, seed, "k_cap > k_max")
    assert picked >= 60 and len(words_hit) == b.legal_words, (picked, words_hit)          # (one_net: 72 picks at reset, none once its envs are done)


# ---- 3. twin equivalence ---------------------------------------------------------------------------------------------------------------
def _prefixes(b, n, R, plen):
    """`plen` legal nets per (env, rollout), highest first and rotated by the rollout; envs with fewer legal nets take what they have."""
    legal = _legal_matrix(b)
    prefix = np.zeros((n, R, max(plen, 1)), np.int32)
    for e in range(n):
        nets = np.flatnonzero(legal[e]) + 1
        for r in range(R if nets.size else 0):
            some = np.roll(nets[::-1], -r)[:plen]
            prefix[e, r, :some.size] = some
    return prefix


def _weighted_twin_equivalence(regions, kw, n, R, at, plens, k_most):
    a = RegionBatch(regions, n_envs=n, device=DEV, **kw)
    a.reset()
    _advance(a, at)
    w = _weights(n, max(a.k_max, 1), 5 + at, zero=0.2)
    compared = 0
    for plen in plens:
        prefix = _prefixes(a, n, R, plen)
        res = _np(a.rollout(R, SEED + plen, policy="weighted", weights=w, prefix=torch.from_numpy(prefix).to(DEV) if plen else None))
        for r in range(R):
            t = RegionBatch(regions, n_envs=n, device=DEV, **kw)
            t.reset()
            _advance(t, at)
            assert t.fetch("hash").cpu().numpy().tobytes() == a.fetch("hash").cpu().numpy().tobytes()
            tw = _play_weighted(t, w, _lib.rollout_seed(SEED + plen, r), k_most, prefix[:, r, :plen] if plen else None)
            _assert_equals_twin(res, r, tw, (at, plen, r))
            compared += n
            t.close()
    return compared


def test_every_weighted_rollout_equals_a_twin_batch_stepped_with_weighted_actions():
    regions = _mixed_regions()
    assert _weighted_twin_equivalence(regions, {}, 24, 3, 2, (0, 1, 2), max(r.n_nets for r in regions)) == 3 * 3 * 24


# ---- 4. oracle parity ------------------------------------------------------------------------------------------------------------------
def test_every_weighted_rollout_equals_the_oracle_replay_of_its_order():
    regions = _mixed_regions()
    n, R = 24, 3
    b, history, reg = _batch_with_history(regions, n, 2)
    nl = b.fetch("nlegal").cpu().numpy()
    res = _np(b.rollout(R, SEED, policy="weighted", weights=_weights(n, b.k_max, 9)))
    assert np.array_equal(res["out"][:, :, 4], np.repeat(nl[:, None], R, 1))          # to the end: every legal net routed
    assert _oracle_check(regions, reg, history, res) == n * R
    assert any(len({tuple(o) for o in res["order"][e].tolist()}) > 1 for e in range(n))          # the seeds differ


# ---- 5. zero-weight nets come last -----------------------------------------------------------------------------------------------------
def test_zero_weight_nets_are_routed_after_every_positive_one():
    regions = _mixed_regions()
    n, R = 24, 3
    b, _, _ = _batch_with_history(regions, n, 1)
    K = b.k_max
    w = _weights(n, K, 21, hi=1000)
    w[:, ::2] = 0
    w[:, 1::2] += 1
    legal = _legal_matrix(b)
    wn = w.cpu().numpy()
    order = b.rollout(R, SEED, policy="weighted", weights=w)["order"].cpu().numpy()
    both = 0
    for e in range(n):
        pos = sum(1 for net in np.flatnonzero(legal[e]) + 1 if wn[e, net - 1] > 0)
        both += int(0 < pos < legal[e].sum())
        for r in range(R):
            nets = [v for v in order[e, r].tolist() if v]
            assert len(nets) == legal[e].sum()
            assert all(wn[e, v - 1] > 0 for v in nets[:pos]) and all(wn[e, v - 1] == 0 for v in nets[pos:]), (e, r, nets)
    assert both >= 8          # envs whose legal nets hold weights of both kinds


# ---- 6. purity -------------------------------------------------------------------------------------------------------------------------
def test_weighted_calls_leave_every_fetchable_array_byte_identical_and_the_inplace_path_alive():
    regions = _mixed_regions()
    kw = dict(n_envs=24, device=DEV, auto_reset=True, max_route_count=1)
    a, t = RegionBatch(regions, **kw), RegionBatch(regions, **kw)
    a.reset(); t.reset()
    obs_a, obs_t = a.alloc_observation().zero_(), t.alloc_observation().zero_()
    a.observation(obs_a); t.observation(obs_t)
    act = torch.empty(24, dtype=torch.int32, device=DEV)
    w = _weights(24, a.k_max, 31, zero=0.3)
    for step in range(8):
        before = _snapshot(a)
        a.weighted_actions(w, SEED + step)
        a.rollout(2, SEED + step, policy="weighted", weights=w)
        if step % 3 == 0:
            a.rollout(2, SEED, policy="weighted", weights=w, max_plies=2, prefix=torch.full((24, 2, 2), 1 + step, dtype=torch.int32, device=DEV))
            a.tree_search(2, 3, SEED + step, sim_weights=w)
        after = _snapshot(a)
        for k in before:
            assert before[k] == after[k], (step, k)
        a.weighted_actions(w, SEED + step, act)
        a.step(act, obs_a, inplace=True)
        t.step(act, obs_t, inplace=True)
        info = a.observe_info()
        assert info["inplace"], (step, info)                                  # the in-place path survived the weighted calls
        assert torch.equal(obs_a, obs_t), step
        for k in ("hash", "record", "owner", "legal", "env_steps"):
            assert a.fetch(k).cpu().numpy().tobytes() == t.fetch(k).cpu().numpy().tobytes(), (step, k)


# ---- 7. refusals, max_plies, done envs; the old entry point unchanged -------------------------------------------------------------------
def test_max_plies_truncates_the_same_weighted_rollout():
    regions = _mixed_regions()
    n, R = 24, 2
    b, history, reg = _batch_with_history(regions, n, 2)
    nl = b.fetch("nlegal").cpu().numpy()
    w = _weights(n, b.k_max, 41)
    full = _np(b.rollout(R, SEED, policy="weighted", weights=w))
    for cap in (1, 3):
        cut = _np(b.rollout(R, SEED, policy="weighted", weights=w, max_plies=cap))
        plies = np.minimum(nl, cap)
        assert np.array_equal(cut["out"][:, :, 4], np.repeat(plies[:, None], R, 1))
        assert np.array_equal(cut["out"][:, :, 5], np.repeat((nl - plies)[:, None], R, 1))
        assert np.array_equal(cut["order"][:, :, :cap], full["order"][:, :, :cap]) and not cut["order"][:, :, cap:].any()
        assert _oracle_check(regions, reg, history, cut, what=cap) == n * R


def test_done_envs_get_action_0_and_the_empty_weighted_rollout():
    regions = _mixed_regions()
    n, R = 24, 2
    b = RegionBatch(regions, n_envs=n, device=DEV, auto_reset=True, max_route_count=1)
    b.reset()
    w = _weights(n, b.k_max, 51)
    act = torch.empty(n, dtype=torch.int32, device=DEV)
    done_seen = live_seen = 0
    for step in range(12):
        nl = b.fetch("nlegal").cpu().numpy()
        h = b.fetch("hash").cpu().numpy()
        res = _np(b.rollout(R, SEED + step, policy="weighted", weights=w))
        a = b.weighted_actions(w, SEED + step, act).cpu().numpy()
        done = nl == 0
        assert np.array_equal(a == 0, done)
        assert not res["out"][done].any() and not res["order"][done].any()
        assert (res["ret"][done].view(np.uint64) == 0).all()                       # +0.0
        assert np.array_equal(res["hash"][done], np.repeat(h[done, None], R, 1))
        assert np.array_equal(res["out"][~done][:, :, 4], np.repeat(nl[~done, None], R, 1))
        assert (res["out"][:, :, 3] & _lib.XR_ENV_WAS_RESET == 0).all()            # never through an auto-reset
        done_seen += int(done.sum()); live_seen += int((~done).sum())
        b.step(act)
    assert done_seen > 0 and live_seen > 0


@pytest.mark.parametrize("kw", [dict(force_scratch_field=True), dict(stream_per_region=True)])
def test_weighted_rollout_and_search_refuse_the_scratch_forms_and_leave_the_batch_untouched(kw):
    regions = [generate_region(3000 + i, dims=(12, 10, 4), k_range=(3, 6)) for i in range(4)]
    b = RegionBatch(regions, device=DEV, **kw)
    b.reset()
    b.step(b.random_actions(SEED))
    w = _ones(b)
    before = _snapshot(b)
    for call in (lambda: b.rollout(2, SEED, policy="weighted", weights=w), lambda: b.tree_search(2, 2, SEED, sim_weights=w)):
        with pytest.raises(_lib.XRouteError) as ei:
            call()
        assert ei.value.code == _lib.XR_ERR_RANGE
    assert torch.equal(b.weighted_actions(w, SEED), b.random_actions(SEED))          # the pick needs no shadow slot: it works on every form
    assert _snapshot(b) == before
    b.step(b.random_actions(SEED + 1))            # still usable


def test_weighted_argument_errors_on_a_live_batch_and_the_old_entry_point_unchanged():
    regions = [generate_region(3000 + i, dims=(12, 10, 4), k_range=(3, 6)) for i in range(4)]
    b = RegionBatch(regions, device=DEV)
    b.reset()
    b.step(b.random_actions(SEED))
    K = b.k_max
    out = torch.empty((4, 2, 8), dtype=torch.int32, device=DEV)
    order = torch.empty((4, 2, K), dtype=torch.int32, device=DEV)
    w = _weights(4, K, 61)
    acts = torch.empty(4, dtype=torch.int32, device=DEV)
    p, po, pw, pa = (C.c_void_p(t.data_ptr()) for t in (out, order, w, acts))
    before = _snapshot(b)
    L = b.L

    def roll(group=-1, R=2, policy=2, out=p, order=None, k_cap=0, weights=pw, wk=K):
        return L.xr_batch_rollout_weighted(b._h, group, R, policy, 7, None, 0, 0, out, None, None, order, k_cap, weights, wk, None)

    for kw, code, word in ((dict(out=None), _lib.XR_ERR_INVALID, b"null"), (dict(group=1), _lib.XR_ERR_INVALID, b"group"),
                           (dict(policy=3), _lib.XR_ERR_INVALID, b"policy"), (dict(policy=-1), _lib.XR_ERR_INVALID, b"policy"),
                           (dict(weights=None), _lib.XR_ERR_INVALID, b"weights_dev"), (dict(wk=K - 1), _lib.XR_ERR_RANGE, b"weights_k_cap"),
                           (dict(R=0), _lib.XR_ERR_RANGE, b"n_rollouts"), (dict(order=po, k_cap=K - 1), _lib.XR_ERR_RANGE, b"k_cap")):
        assert roll(**kw) == code, kw
        msg = L.xr_last_error()
        assert b"xr_batch_rollout_weighted" in msg and word in msg, (kw, msg)
    for args, code, word in (((-1, None, K, pa), _lib.XR_ERR_INVALID, b"null"), ((-1, pw, K, None), _lib.XR_ERR_INVALID, b"null"),
                             ((1, pw, K, pa), _lib.XR_ERR_INVALID, b"group"), ((-2, pw, K, pa), _lib.XR_ERR_INVALID, b"group"),
                             ((-1, pw, K - 1, pa), _lib.XR_ERR_RANGE, b"k_cap")):
        assert L.xr_batch_weighted_actions(b._h, *args, 7, None) == code, args
        msg = L.xr_last_error()
        assert b"xr_batch_weighted_actions" in msg and word in msg, (args, msg)
    # the old entry point keeps refusing policy 2, under its own name
    assert L.xr_batch_rollout(b._h, -1, 2, 2, 7, None, 0, 0, p, None, None, None, 0, None) == _lib.XR_ERR_INVALID
    assert b"xr_batch_rollout:" in L.xr_last_error() and b"policy" in L.xr_last_error()
    assert _snapshot(b) == before
    # policies 0 and 1 through the new entry point are xr_batch_rollout exactly; the weights are not looked at (null, or a short k_cap)
    want = _np(b.rollout(2, 7))
    assert roll(policy=1, weights=None, wk=0) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want["out"])
    prefix = torch.from_numpy(_prefixes(b, 4, 2, 2)).to(DEV)
    want = _np(b.rollout(2, 7, policy="stop", prefix=prefix))
    assert L.xr_batch_rollout_weighted(b._h, -1, 2, 0, 7, C.c_void_p(prefix.data_ptr()), 2, 0, p, None, None, po, K, pw, 0, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want["out"]) and np.array_equal(order.cpu().numpy(), want["order"])
    # a wider weight table: the columns beyond k_max are never read
    wide = torch.full((4, K + 3), 2 ** 31 - 1, dtype=torch.int32, device=DEV)
    wide[:, :K] = w
    assert roll(weights=C.c_void_p(wide.data_ptr()), wk=K + 3) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), _np(b.rollout(2, 7, policy="weighted", weights=w))["out"])
    assert _snapshot(b) == before
    b.step(b.random_actions(SEED + 1))            # still usable


# ---- 8. env groups ---------------------------------------------------------------------------------------------------------------------
def test_groups_sample_and_roll_out_on_their_own_streams_like_the_whole_batch():
    regions = [generate_region(3000 + i) for i in range(8)] + _mixed_regions()[:6]
    n, R = 40, 2
    b = RegionBatch(regions, n_envs=n, device=DEV)
    b.set_groups([0, 13, 40])
    b.reset()
    _advance(b, 2)
    w = _weights(n, b.k_max, 71, zero=0.2)
    whole_act = b.weighted_actions(w, SEED).cpu().numpy()
    whole = _np(b.rollout(R, SEED, policy="weighted", weights=w))
    tree = _np(b.tree_search(2, 2, SEED, sim_weights=w))
    torch.cuda.synchronize()
    cur = torch.cuda.current_stream()
    streams = [torch.cuda.Stream() for _ in range(2)]
    got = {}
    for g, s in enumerate(streams):
        s.wait_stream(cur)
        lo, hi = b.group_bounds(g)
        wg = w[lo:hi].contiguous()
        with torch.cuda.stream(s):
            got[g] = (b.weighted_actions(wg, SEED, group=g, stream=s), b.rollout(R, SEED, policy="weighted", weights=wg, group=g, stream=s),
                      b.tree_search(2, 2, SEED, sim_weights=wg, group=g, stream=s))
    for s in streams:
        cur.wait_stream(s)
    torch.cuda.synchronize()
    for g in range(2):
        lo, hi = b.group_bounds(g)
        act, res, tr = got[g]
        assert np.array_equal(act.cpu().numpy(), whole_act[lo:hi]), g
        _assert_same_rollouts(_np(res), {k: v[lo:hi] for k, v in whole.items()}, g)
        tr = _np(tr)
        for k in ("visits", "info", "best_order"):
            assert np.array_equal(tr[k], tree[k][lo:hi]), (g, k)
        assert np.array_equal(tr["best_return"].view(np.uint64), tree["best_return"][lo:hi].view(np.uint64)), g


# ---- 9. router variants ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["auto", "sweep", "dial", "dial_r2", "v2_guides"])
def test_weighted_rollout_under_every_router_variant(variant):
    if variant == "v2_guides":
        regions = _pack(slice(5, 200, 13))[:8]
        assert all(r.guide_off is not None and r.guide_off[-1] > 0 for r in regions)
        kw = dict(guide_cost=1000, guide_margin=1, maze_end_iter=3)
    else:
        regions = [generate_region(3000 + i) for i in range(8)]
        kw = dict(router={"auto": 0, "sweep": 1, "dial": 2, "dial_r2": 3}[variant], dial_mult=0 if variant != "dial" else 5)
    n = len(regions)
    assert _weighted_twin_equivalence(regions, kw, n, 2, 3, (1,), max(r.n_nets for r in regions)) == 2 * n


# ---- 10. tree search -------------------------------------------------------------------------------------------------------------------
TREE_FIELDS = ("paths", "returns", "visits", "value", "info", "best_order", "best_return")


def _assert_same_search(a, t, what):
    for k in TREE_FIELDS:
        x, y = a[k], t[k]
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k, x.shape, y.shape, x.dtype, y.dtype)
        if x.dtype == np.float64:
            x, y = x.view(np.uint64), y.view(np.uint64)
        assert np.array_equal(x, y), (what, k, np.argwhere(x != y)[:4].tolist())


def test_weighted_tree_search_against_the_plain_search_and_the_twin():
    regions = _mixed_regions()
    n, W, P = 6, 3, 4
    b = RegionBatch(regions, n_envs=n, device=DEV)
    b.reset()
    _advance(b, 1)
    K = max(b.k_max, 1)
    plain = _np(b.tree_search(W, P, SEED, trace=True))
    # NULL sim_weights through the new entry point, and unit sim_weights: xr_batch_tree_search exactly
    res = {k: torch.empty_like(torch.from_numpy(v)).to(DEV) for k, v in plain.items()}
    ptr = {k: C.c_void_p(v.data_ptr()) for k, v in res.items()}
    assert b.L.xr_batch_tree_search_weighted(b._h, -1, W, P, C.c_uint64(SEED), None, 1 + W * P * K, 1.25, 19652.0, ptr["visits"], ptr["value"], K, ptr["info"],
                                             ptr["best_order"], ptr["best_return"], ptr["paths"], ptr["returns"], None, None) == 0
    torch.cuda.synchronize()
    _assert_same_search(_np(res), plain, "NULL sim_weights")
    _assert_same_search(_np(b.tree_search(W, P, SEED, trace=True, sim_weights=_ones(b))), plain, "unit sim_weights")
    # random sim_weights and a prior: the spec's twin, its evaluate the weighted rollout below the wave's paths
    w = _weights(n, K, 81, zero=0.25)
    g = torch.Generator().manual_seed(82)
    prior = torch.rand((n, K), generator=g, dtype=torch.float32).to(DEV).contiguous()
    before = _snapshot(b)
    dev = _np(b.tree_search(W, P, SEED, prior=prior, trace=True, sim_weights=w))
    assert _snapshot(b) == before
    legal = [(np.flatnonzero(row) + 1).tolist() for row in _legal_matrix(b)]
    E = _lib.tree_exploration_table(1.25, 19652.0, W * P)

    def evaluate(wave, paths):
        prefix = np.zeros((n, P, K), np.int32)
        for r in range(n):
            for j in range(P):
                prefix[r, j, :len(paths[r][j])] = paths[r][j]
        res = b.rollout(P, _lib.tree_seed(SEED, wave), policy="weighted", weights=w, prefix=torch.from_numpy(prefix).to(DEV))
        return res["ret"].cpu().numpy().tolist(), res["order"].cpu().numpy().tolist()

    results, paths, returns, trees = tree_twin.search(legal, W, P, 1 + W * P * K, E, evaluate, K, prior.cpu().numpy().tolist())
    tw = dict(paths=np.array(paths, np.int32).reshape(n, W * P, K), returns=np.array(returns, np.float64).reshape(n, W * P),
              visits=np.array([r["visits"] for r in results], np.int32), value=np.array([r["value"] for r in results], np.float64),
              info=np.array([r["info"] for r in results], np.int32), best_order=np.array([r["best_order"] for r in results], np.int32),
              best_return=np.array([r["best_return"] for r in results], np.float64))
    _assert_same_search(dev, tw, "random sim_weights")
    assert max(t.max_depth for t in trees) >= 2 and not np.array_equal(dev["returns"], plain["returns"])          # the inputs bite


# ---- 11. CEM ---------------------------------------------------------------------------------------------------------------------------
def test_cem_search_improves_monotonically_and_returns_an_order_that_replays_to_its_return():
    regions = _mixed_regions()
    n, R = 24, 8
    b = RegionBatch(regions, n_envs=n, device=DEV)
    b.reset()
    _advance(b, 1)
    before = _snapshot(b)
    # one iteration is the best of the same R random rollouts
    order1, ret1, hist1 = cem_search(b, 1, R, 3, SEED)
    rnd = _np(b.rollout(R, SEED))
    first = np.argmax(rnd["ret"], axis=1)                                         # (np.argmax: the first maximum)
    assert np.array_equal(order1.cpu().numpy(), rnd["order"][np.arange(n), first])
    assert np.array_equal(ret1.cpu().numpy().view(np.uint64), rnd["ret"][np.arange(n), first].view(np.uint64))
    assert hist1.shape == (1, n) and torch.equal(hist1[0], ret1)
    order, ret, hist = cem_search(b, 4, R, 3, SEED)
    assert _snapshot(b) == before
    h = hist.cpu().numpy()
    assert h.shape == (4, n) and (np.diff(h, axis=0) >= 0).all()                   # the best-ever return never decreases
    assert np.array_equal(h[0].view(np.uint64), ret1.cpu().numpy().view(np.uint64)) and np.array_equal(h[-1], ret.cpu().numpy())
    # the returned order, stepped on a twin, gives the returned return bit for bit
    t = RegionBatch(regions, n_envs=n, device=DEV)
    t.reset()
    _advance(t, 1)
    on = order.cpu().numpy()
    total = np.zeros(n, np.float64)
    for j in range(on.shape[1]):
        col = np.ascontiguousarray(on[:, j])
        if not col.any():
            break
        t.step(torch.from_numpy(col).to(DEV))
        rec = t.records()
        live = col > 0
        assert not (rec["status"][live] & BAD).any()
        total[live] = total[live] + rec["reward"][live]
    assert (t.fetch("nlegal").cpu().numpy() == 0).all()
    assert np.array_equal(total.view(np.uint64), ret.cpu().numpy().view(np.uint64))


# ---- 12. full size ---------------------------------------------------------------------------------------------------------------------
def test_weighted_rollouts_at_4096_ispd18_slots_equal_what_the_batch_then_does():
    b = RegionBatch(_pack(), n_envs=4096, device=DEV, auto_reset=False)
    b.reset()
    _advance(b, 3)
    w = _weights(4096, b.k_max, 91, zero=0.2)
    res = b.rollout(2, SEED, policy="weighted", weights=w)
    first = b.weighted_actions(w, _lib.rollout_seed(SEED, 0))
    assert torch.equal(res["order"][:, 0, 0], first)
    res = _np(res)
    tw = _play_weighted(b, w, _lib.rollout_seed(SEED, 1), b.k_max)
    _assert_equals_twin(res, 1, tw, "4096 slots")
    assert tw["plies"].sum() > 4096
