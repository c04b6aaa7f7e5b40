"""Lookahead on the MI355X (xr_batch_lookahead / RegionBatch.lookahead / XRouteVectorEnv.lookahead, greedy_actions): every candidate net of
every env priced from the current state without stepping.  Oracle parity for EVERY (env, legal net) pair; purity (every fetchable array
byte-identical, twin batches with identical hash chains, the in-place observation path kept); consistency with the step at 4096
ispd18_test1 slots; every router variant; candidate masks; env groups on their own streams; the vector env's greedy policy."""
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
SEED = 0x10CA
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEG_INF_BITS = np.array([-np.inf]).view(np.uint64)[0]


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
    from tests.helpers import obs_set_regions
    extra = [generate_region(9100 + i, dims=d, k_range=(4, 10), pins=(3, 5), net_span=7)
             for i, d in enumerate([(16, 12, 5), (20, 14, 6), (13, 17, 4), (24, 20, 5)])]
    return obs_set_regions("mixed") + extra


def _snapshot(b):
    """Every array xr_batch_fetch returns, as bytes."""
    return {k: b.fetch(k).cpu().numpy().tobytes() for k in b._FETCH}


def _legal_matrix(b, legal=None):
    """bool [n_envs, k_max]: net n (column n - 1) is legal."""
    words = (b.fetch("legal") if legal is None else legal).cpu().numpy().view(np.uint64)
    bits = ((words[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).astype(bool)
    return bits.reshape(words.shape[0], -1)[:, :max(b.k_max, 1)]


def _assert_fill(ds, rw, cand, what=""):
    """Entries that are no candidates hold {0, 0, 0, -1} / -inf; candidates hold a status >= 0 and a finite reward."""
    ds, rw = ds.cpu().numpy(), rw.cpu().numpy()
    assert ds.shape[:2] == cand.shape and rw.shape == cand.shape, (what, ds.shape, rw.shape, cand.shape)
    assert (ds[~cand] == np.array([0, 0, 0, -1], np.int32)).all(), what
    assert (rw[~cand].view(np.uint64) == NEG_INF_BITS).all(), what
    assert (ds[cand][:, 3] >= 0).all() and np.isfinite(rw[cand]).all(), what
    return ds, rw


def _step_and_check(b, ds, rw, act, obs=None, inplace=False):
    """Step `b` with `act`; what every env publishes equals the lookahead entry (ds, rw: numpy, taken just before) of its action."""
    nl_before = b.fetch("nlegal").cpu().numpy()
    b.step(act, obs, inplace=inplace) if obs is not None else b.step(act)
    rec = b.records()
    a = act.cpu().numpy()
    live = np.flatnonzero(nl_before > 0)
    assert (a[live] >= 1).all()
    e = ds[live, a[live] - 1]
    assert np.array_equal(e[:, :3], rec["delta"][live]), "delta"
    assert np.array_equal(e[:, 3], rec["status"][live].astype(np.int32)), "status"
    assert np.array_equal(rw[live, a[live] - 1].view(np.uint64), rec["reward"][live].view(np.uint64)), "reward bits"
    return live.size


# ---- 1. oracle parity, nothing left out ------------------------------------------------------------------------------------------
def test_lookahead_equals_the_oracle_for_every_env_and_every_legal_net():
    from oracle import xr_oracle as orc
    regions = _mixed_regions()
    n = 24
    b = RegionBatch(regions, n_envs=n, device=DEV)
    b.reset()
    reg = b.fetch("region").cpu().numpy()
    history = [[] for _ in range(n)]
    compared = expected = 0
    for step in range(6):
        if step in (0, 2, 5):
            ds, rw = b.lookahead()
            legal = _legal_matrix(b)
            nl = b.fetch("nlegal").cpu().numpy()
            assert np.array_equal(legal.sum(1), nl)
            ds, rw = _assert_fill(ds, rw, legal, f"step {step}")
            expected += int(nl.sum())
            for e in range(n):
                for net in (np.flatnonzero(legal[e]) + 1).tolist():
                    env = orc.OracleEnv(regions[int(reg[e])])
                    env.reset()
                    for a in history[e]:
                        env.step(a)
                    ref = env.step(net)
                    got = ds[e, net - 1]
                    assert got[:3].tolist() == ref["delta"].tolist(), (step, e, net, got, ref["delta"])
                    assert int(got[3]) == ref["status"], (step, e, net, got[3], ref["status"])
                    want = np.array([orc.reward(*[int(v) for v in ref["delta"]])]).view(np.uint64)[0]
                    assert rw[e, net - 1:net].view(np.uint64)[0] == want, (step, e, net)
                    compared += 1
        act = b.random_actions(SEED + step)
        b.step(act)
        for e, a in enumerate(act.cpu().numpy().tolist()):
            if a:
                history[e].append(a)
    assert compared == expected and compared > 100, (compared, expected)


# ---- 2. purity -------------------------------------------------------------------------------------------------------------------
def test_lookahead_leaves_every_fetchable_array_byte_identical():
    regions = _mixed_regions()
    b = RegionBatch(regions, n_envs=24, device=DEV, auto_reset=True, max_route_count=1)
    b.reset()
    act = torch.empty(24, dtype=torch.int32, device=DEV)
    for step in range(12):
        before = _snapshot(b)
        b.lookahead()
        if step % 3 == 0:
            b.lookahead(mask=torch.full((24, b.legal_words), 0x5555555555555555, dtype=torch.int64, device=DEV))
        after = _snapshot(b)
        for k in before:
            assert before[k] == after[k], (step, k)
        b.step(b.random_actions(SEED + step, act))


@pytest.mark.parametrize("mode", ["route", "inplace", "inplace_u8"])
def test_a_batch_that_looks_ahead_every_step_equals_its_twin_that_never_does(mode):
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
    checked = 0
    for step in range(50):
        ds, rw = a.lookahead()
        ds, rw = _assert_fill(ds, rw, _legal_matrix(a), f"step {step}")
        a.random_actions(SEED + step, act)
        checked += _step_and_check(a, ds, rw, act, obs_a, inplace=True)
        t.step(act, obs_t, inplace=True) if obs_t is not None else t.step(act)
        for k in ("hash", "record", "owner", "legal", "region", "replay", "env_steps", "steps", "path", "path_len", "sweeps"):
            assert a.fetch(k).cpu().numpy().tobytes() == t.fetch(k).cpu().numpy().tobytes(), (step, k)
        if obs_a is not None:
            info = a.observe_info()
            assert info["form"] == 3 and info["inplace"], (step, info)          # mode | 16: the in-place path survived the lookahead
            assert torch.equal(obs_a, obs_t), step
    assert checked > 600


# ---- 3. consistency at full size -------------------------------------------------------------------------------------------------
def test_lookahead_at_4096_ispd18_slots_prices_the_action_every_env_then_takes():
    b = RegionBatch(_pack(), n_envs=4096, device=DEV, auto_reset=True)
    b.reset()
    act = torch.empty(4096, dtype=torch.int32, device=DEV)
    for step in range(25):                       # towards the stationary nets-left distribution: envs finish and restart at different times
        b.step(b.random_actions(SEED + step, act))
    done_seen = checked = 0
    for step in range(25, 33):
        ds, rw = b.lookahead()
        legal = _legal_matrix(b)
        nl = b.fetch("nlegal").cpu().numpy()
        assert np.array_equal(legal.sum(1), nl)
        ds, rw = _assert_fill(ds, rw, legal, f"step {step}")
        done_seen += int((nl == 0).sum())          # (their rows: all -1, by _assert_fill)
        b.random_actions(SEED + step, act)
        checked += _step_and_check(b, ds, rw, act)
    assert checked > 8 * 3500 and done_seen > 0, (checked, done_seen)


# ---- 4. variants -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["auto", "sweep", "dial", "dial_r2", "v2_guides"])
def test_lookahead_under_every_router_variant(variant):
    if variant == "v2_guides":
        regions = _pack(slice(5, 200, 13))
        assert all(r.guide_off is not None and r.guide_off[-1] > 0 for r in regions)
        kw = dict(guide_cost=1000, guide_margin=1, maze_end_iter=3)
    else:
        regions = [generate_region(3000 + i) for i in range(12)]
        kw = dict(router={"auto": 0, "sweep": 1, "dial": 2, "dial_r2": 3}[variant], dial_mult=0 if variant != "dial" else 5)
    n = 2 * len(regions)
    kw.update(n_envs=n, device=DEV, auto_reset=True, max_route_count=1)
    a, t = RegionBatch(regions, **kw), RegionBatch(regions, **kw)
    a.reset(); t.reset()
    act = torch.empty(n, dtype=torch.int32, device=DEV)
    checked = 0
    for step in range(14):
        ds, rw = a.lookahead()
        ds, rw = _assert_fill(ds, rw, _legal_matrix(a), f"{variant} step {step}")
        a.random_actions(SEED + step, act)
        checked += _step_and_check(a, ds, rw, act)
        t.step(act)
        for k in ("hash", "record", "owner", "legal"):
            assert a.fetch(k).cpu().numpy().tobytes() == t.fetch(k).cpu().numpy().tobytes(), (variant, step, k)
    assert checked > 10 * n


@pytest.mark.parametrize("kw", [dict(force_scratch_field=True), dict(stream_per_region=True)])
def test_lookahead_refuses_the_scratch_forms_and_leaves_the_batch_untouched(kw):
    regions = [generate_region(3000 + i, dims=(12, 10, 4), k_range=(3, 6)) for i in range(4)]
    b = RegionBatch(regions, device=DEV, **kw)
    b.reset()
    b.step(b.random_actions(SEED))
    before = _snapshot(b)
    with pytest.raises(_lib.XRouteError) as ei:
        b.lookahead()
    assert ei.value.code == _lib.XR_ERR_RANGE
    assert _snapshot(b) == before
    b.step(b.random_actions(SEED + 1))            # still usable


def test_lookahead_argument_errors_on_a_live_batch():
    import ctypes as C
    regions = [generate_region(3000 + i, dims=(12, 10, 4), k_range=(3, 6)) for i in range(4)]
    b = RegionBatch(regions, device=DEV)
    b.reset()
    out = torch.empty((4, b.k_max, 4), dtype=torch.int32, device=DEV)
    p = C.c_void_p(out.data_ptr())
    before = _snapshot(b)
    L = b.L
    assert L.xr_batch_lookahead(b._h, -1, None, None, b.k_max, None, None) == _lib.XR_ERR_INVALID
    assert L.xr_batch_lookahead(b._h, 1, None, p, b.k_max, None, None) == _lib.XR_ERR_INVALID
    assert L.xr_batch_lookahead(b._h, -2, None, p, b.k_max, None, None) == _lib.XR_ERR_INVALID
    assert L.xr_batch_lookahead(b._h, -1, None, p, b.k_max - 1, None, None) == _lib.XR_ERR_RANGE
    assert b"k_cap" in L.xr_last_error()
    assert _snapshot(b) == before
    with pytest.raises(ValueError):
        b.lookahead(out=out.to(torch.int64))
    with pytest.raises(ValueError):
        b.lookahead(mask=torch.zeros((4, b.legal_words), dtype=torch.int32, device=DEV))
    # reward_out is optional in the C ABI; a wider k_cap pads rows with non-candidates
    wide = torch.full((4, b.k_max + 3, 4), 77, dtype=torch.int32, device=DEV)
    assert L.xr_batch_lookahead(b._h, -1, None, C.c_void_p(wide.data_ptr()), b.k_max + 3, None, None) == 0
    ds, _ = b.lookahead()
    assert torch.equal(wide[:, :b.k_max], ds)
    assert (wide[:, b.k_max:].cpu().numpy() == np.array([0, 0, 0, -1], np.int32)).all()


# ---- 5. mask ---------------------------------------------------------------------------------------------------------------------
def test_a_candidate_mask_evaluates_exactly_legal_and_mask():
    from tests.helpers import OBS_MANY_NETS
    regions = _mixed_regions() + [generate_region(9300, **OBS_MANY_NETS)]         # (a region with 200+ nets: several legal words)
    n = len(regions)
    b = RegionBatch(regions, n_envs=n, device=DEV)
    assert b.legal_words >= 4
    b.reset()
    rng = np.random.default_rng(11)
    for step in range(4):
        full_ds, full_rw = b.lookahead()
        legal = _legal_matrix(b)
        full_ds, full_rw = _assert_fill(full_ds, full_rw, legal)
        m = rng.integers(0, 1 << 63, size=(n, b.legal_words), dtype=np.int64) | (rng.integers(0, 2, size=(n, b.legal_words), dtype=np.int64) << 63)
        if step == 3:
            m[::2] = 0                              # nothing asked for: only -1 rows
        mask = torch.from_numpy(m).to(DEV)
        ds, rw = b.lookahead(mask=mask)
        cand = legal & _legal_matrix(b, mask)
        ds, rw = _assert_fill(ds, rw, cand, f"masked, step {step}")
        assert 0 < cand.sum() < legal.sum()
        assert np.array_equal(ds[cand], full_ds[cand])
        assert np.array_equal(rw[cand].view(np.uint64), full_rw[cand].view(np.uint64))
        b.step(b.random_actions(SEED + step))


# ---- 6. groups -------------------------------------------------------------------------------------------------------------------
def test_groups_look_ahead_on_their_own_streams_between_steps_of_other_groups():
    regions = [generate_region(3000 + i) for i in range(8)] + _mixed_regions()[:6]
    n = 40
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
                    results[g].append(a.lookahead(group=g, stream=s))          # count = steps taken so far by this group
                    act = a.random_actions_group(g, SEED, stream=s)
                    a.step_group(g, act, stream=s)
    for s in streams:
        cur.wait_stream(s)
    torch.cuda.synchronize()
    # lock-step twin: whole-batch lookahead before every step
    twin = []
    act = torch.empty(n, dtype=torch.int32, device=DEV)
    for i in range(rounds * max(cadence)):
        ds, rw = t.lookahead()
        twin.append((ds.cpu().numpy(), rw.cpu().numpy()))
        t.step(t.random_actions(SEED, act))
    for g in range(4):
        lo, hi = a.group_bounds(g)
        assert len(results[g]) == rounds * cadence[g]
        for i, (ds, rw) in enumerate(results[g]):
            assert tuple(ds.shape) == (hi - lo, a.k_max, 4)
            assert np.array_equal(ds.cpu().numpy(), twin[i][0][lo:hi]), (g, i)
            assert np.array_equal(rw.cpu().numpy().view(np.uint64), twin[i][1][lo:hi].view(np.uint64)), (g, i)


# ---- 7. vector env ---------------------------------------------------------------------------------------------------------------
def test_vector_env_greedy_actions_and_a_greedy_episode():
    from xroute_env_amd.envs.vector_env import XRouteVectorEnv
    regions = _mixed_regions()
    env = XRouteVectorEnv(regions, n_envs=24, device=DEV, max_route_count=1)
    env.reset()
    k_most = max(r.n_nets for r in regions)
    finished = np.zeros(24, bool)
    for step in range(k_most + 2):
        _, rw = env.lookahead()
        act = env.greedy_actions()
        r = rw.cpu().numpy()
        want = np.where(np.isneginf(r).all(1), 0, np.argmax(r, axis=1) + 1)          # (np.argmax: the first maximum)
        assert act.dtype == torch.int32 and np.array_equal(act.cpu().numpy(), want), step
        nl = env.batch.fetch("nlegal").cpu().numpy()
        assert np.array_equal(act.cpu().numpy() == 0, nl == 0)
        _, _, done, info = env.step(act)
        rec = env.batch.records()
        live = nl > 0
        assert not (rec["status"][live] & _lib.XR_ENV_BAD_ACTION).any(), step
        finished |= done.cpu().numpy().astype(bool)
    assert finished.all()


def test_vector_env_group_lookahead_runs_on_the_groups_stream():
    from xroute_env_amd.envs.vector_env import XRouteVectorEnv
    regions = _mixed_regions()
    env = XRouteVectorEnv(regions, n_envs=24, device=DEV, max_route_count=1, groups=3, with_observation=False)
    env.reset()
    whole = env.greedy_actions().cpu().numpy()
    for g in range(3):
        lo, hi = env.batch.group_bounds(g)
        act = env.greedy_actions(g)
        env.step_wait(g)
        assert np.array_equal(act.cpu().numpy(), whole[lo:hi])
        env.step_async(act, g)
    env.step_wait()
    torch.cuda.synchronize()
