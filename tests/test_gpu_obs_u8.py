"""uint8 observations on the MI355X (xr_batch_step_observe_u8 / xr_batch_observation_u8): every byte equals the fp32 observation's float
cast to a byte, for the stand-alone writer and for the queue form of the step (full write and in place, aligned and unaligned planes,
env groups, config-5-sized regions, 4096 slots); the step side equals an fp32 twin; refusals leave a live batch untouched; the vector env
and the agents take the byte grid."""
import ctypes as C
import dataclasses
import gc
import hashlib
import os

import numpy as np
import pytest
import torch

from tests.helpers import assert_rows_match_oracle
from xroute_env_amd import _lib
from xroute_env_amd.batch import RegionBatch
from xroute_env_amd.regions import config_regions, generate_region

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x0B58
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
STATE = ("hash", "cum", "delta", "reward", "done", "legal", "region", "replay", "env_steps", "nlegal", "record")


@pytest.fixture(autouse=True)
def _release_cached_memory():
    """Hand the observation buffers of every test back to the driver: a later test that allocates with torch.empty and compares whole
    rows (bytes past an env's (2+7K)*N included) must not inherit these tests' bytes from the caching allocator."""
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _pack(n):
    from xroute_env_amd.lefdef import load_region_pack
    return load_region_pack(os.path.join(GOLDEN, "ispd18_test1_regions.npz"))[:n]


def _lens(batch, lo=0, hi=None):
    hi = batch.n_envs if hi is None else hi
    reg = batch.fetch("region")[lo:hi].cpu().numpy()
    nl = batch.fetch("nlegal")[lo:hi].cpu().numpy()
    return [(2 + 7 * int(nl[i])) * batch.regions[int(reg[i])].n_nodes for i in range(hi - lo)]


def _assert_rows_cast(u8, f32, lens, what):
    """u8 rows == fp32 rows cast to bytes over every env's (2+7K)*N prefix."""
    u, f = u8.cpu().numpy(), f32.cpu().numpy()
    for i, n in enumerate(lens):
        fr = f[i, :n]
        assert (fr == np.round(fr)).all() and fr.min(initial=0) >= 0 and fr.max(initial=0) <= 255, (what, i)
        assert np.array_equal(u[i, :n], fr.astype(np.uint8)), (what, "row", i)


def _state(batch):
    return {k: batch.fetch(k).cpu().numpy().copy() for k in STATE}


def _assert_state_equal(a, b, what):
    for k in STATE:
        assert np.array_equal(a[k], b[k]), (what, k)


def _make(regions, n_envs, **kw):
    return RegionBatch(regions, n_envs=n_envs, device=DEV, auto_reset=True, max_route_count=1, **kw)


# ---- 1. stand-alone observation -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(24, 40, 9), (5, 7, 3), (1, 1, 1), (3, 1, 5), (17, 2, 2), (7, 9, 5)])
def test_observation_u8_equals_fp32_and_oracle(dims):
    from oracle import xr_oracle as orc
    regions = [generate_region(6000 + i + dims[0], dims=dims, k_range=(1, 12), net_span=5) for i in range(10)]
    batch = RegionBatch(regions, device=DEV)
    envs = [orc.OracleEnv(r) for r in regions]
    batch.reset()
    for step in range(6):
        f = batch.observation()
        u = batch.observation(batch.alloc_observation(dtype=torch.uint8))
        assert u.dtype == torch.uint8 and u.shape[1] == batch.obs_env_stride_u8 and batch.obs_env_stride_u8 % 128 == 0
        _assert_rows_cast(u, f, _lens(batch), (dims, step))
        un = u.cpu().numpy()
        for i, env in enumerate(envs):
            ro = env.observation()
            assert np.array_equal(ro.ravel().astype(np.uint8), un[i, :ro.size]), (dims, step, i)
        legal = batch.legal_sets()
        acts = [sorted(s)[len(s) // 2] if s else 0 for s in legal]
        batch.step(torch.tensor(acts, dtype=torch.int32, device=DEV))
        for i, env in enumerate(envs):
            if acts[i]:
                env.step(acts[i])


def test_observation_u8_subrange_and_wide_stride():
    regions = [generate_region(6100 + i, dims=(6, 5, 4), k_range=(2, 4)) for i in range(7)]
    batch = RegionBatch(regions, device=DEV)
    batch.reset()
    full = batch.observation()
    out = torch.full((3, batch.obs_env_stride_u8 + 48), 0xAB, dtype=torch.uint8, device=DEV)
    batch.observation(out, env_lo=2, env_hi=5)
    lens = _lens(batch, 2, 5)
    _assert_rows_cast(out, full[2:5], lens, "subrange")
    for j, n in enumerate(lens):
        assert (out[j, n:] == 0xAB).all()              # nothing written past the env's own channels


# ---- 2. the step equals an fp32 twin ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inplace", [0, 1])
@pytest.mark.parametrize("which", ["aligned", "ispd18_pack"])
def test_step_u8_equals_fp32_twin(which, inplace):
    regions = [generate_region(8100 + i, dims=(16, 10, 4), k_range=(2, 6), net_span=5) for i in range(6)] if which == "aligned" else _pack(12)
    if which == "ispd18_pack":
        assert any(r.n_nodes % 16 for r in regions)
    n = 20
    a, b = _make(regions, n), _make(regions, n)
    fa = a.alloc_observation().zero_()
    ub = b.alloc_observation(dtype=torch.uint8).zero_()
    for x, o in ((a, fa), (b, ub)):
        x.reset(rotate=True)
        x.observation(o)
    act = torch.empty(n, dtype=torch.int32, device=DEV)
    act_b = torch.empty(n, dtype=torch.int32, device=DEV)
    seen = set()
    for t in range(30):
        a.random_actions(SEED, act)
        b.random_actions(SEED, act_b)
        assert torch.equal(act, act_b)
        a.step(act, fa, inplace=bool(inplace))
        b.step(act, ub, inplace=bool(inplace))
        info = b.observe_info()
        assert info["form"] == _lib_queue() and info["inplace"] == bool(inplace)
        _assert_state_equal(_state(a), _state(b), (which, inplace, t))
        assert a.legal_sets() == b.legal_sets()
        _assert_rows_cast(ub, fa, _lens(a), (which, inplace, t))
        # and both against the oracle, not only against each other; the buffers started as zeros and are not refilled between steps, so
        # older planes may remain up to the longest row: behind that, stride padding included, the zeros must still be there
        assert_rows_match_oracle(b, ub, 0, n, 0, False, (which, inplace, t, "u8"))
        assert_rows_match_oracle(a, fa, 0, n, 0.0, False, (which, inplace, t, "fp32"))
        seen.add(tuple(a.fetch("region").cpu().tolist()))
    assert len(seen) > 1                            # episodes ended, auto-reset and rotated on the way


def _lib_queue():
    return 3            # XR_OBS_QUEUE


# ---- 3. in-place fallbacks --------------------------------------------------------------------------------------------------------
def test_u8_inplace_falls_back_to_full_write():
    """u8 in place after a buffer swap, a whole-batch fp32 call, an fp32 write to the same address (same stride number) and a reset:
    each time a full write, byte-identical to a u8 full-write twin."""
    regions = [generate_region(8200 + i, dims=(16, 10, 4), k_range=(3, 6), net_span=5) for i in range(5)]
    n = 16
    a, b = _make(regions, n), _make(regions, n)
    S = a.obs_env_stride                            # floats for fp32, bytes for u8: the same number, the same address
    raw = torch.zeros(n * S * 4, dtype=torch.uint8, device=DEV)
    ua = raw[:n * S].view(n, S)
    fa_same = raw.view(torch.float32).view(n, S)
    ua2 = a.alloc_observation(dtype=torch.uint8).zero_()
    f_other = a.alloc_observation()
    f_twin = b.alloc_observation()
    ub = b.alloc_observation(dtype=torch.uint8)
    act = torch.empty(n, dtype=torch.int32, device=DEV)
    for x in (a, b):
        x.reset(rotate=True)
    a.observation(ua)

    def step_both(buf_a, expect_inplace):
        a.random_actions(SEED, act)
        a.step(act, buf_a, inplace=True)
        assert a.observe_info()["inplace"] == expect_inplace
        b.step(act, ub)
        _assert_state_equal(_state(a), _state(b), "state")
        lens = _lens(b)
        ua_n, ub_n = buf_a.cpu().numpy(), ub.cpu().numpy()
        for i, m in enumerate(lens):
            assert np.array_equal(ua_n[i, :m], ub_n[i, :m]), ("row", i)

    step_both(ua, True)
    step_both(ua, True)
    step_both(ua2, False)                           # buffer swap
    step_both(ua2, True)
    a.random_actions(SEED, act)                     # a whole-batch fp32 call on both
    a.step(act, f_other)
    b.step(act, f_twin)
    step_both(ua2, False)
    step_both(ua2, True)
    step_both(ua, False)                            # (ua went stale at the swap)
    a.observation(fa_same)                          # fp32 write to ua's address, same stride number
    step_both(ua, False)
    step_both(ua, True)
    for x in (a, b):                                # reset
        x.reset(rotate=True)
    step_both(ua, False)
    step_both(ua, True)


# ---- 4. groups ----------------------------------------------------------------------------------------------------------------------
def test_u8_group_steps_equal_lockstep():
    regions = [generate_region(8300 + i, dims=(7, 9, 5), k_range=(2, 5), net_span=5) for i in range(5)]
    bounds = [0, 1, 7, 13, 24]
    n = bounds[-1]
    a, b = _make(regions, n), _make(regions, n)
    a.set_groups(bounds)
    ua, ub = a.alloc_observation(dtype=torch.uint8).zero_(), b.alloc_observation(dtype=torch.uint8).zero_()
    for x, o in ((a, ua), (b, ub)):
        x.reset(rotate=True)
        x.observation(o)
    cur = torch.cuda.current_stream()
    streams = [torch.cuda.Stream() for _ in range(4)]
    acts = []
    for g, s in enumerate(streams):
        s.wait_stream(cur)
        with torch.cuda.stream(s):
            acts.append(torch.empty(bounds[g + 1] - bounds[g], dtype=torch.int32, device=DEV))
    cadence = [1, 2, 3, 4]
    for rnd in range(6):
        for k in range(4):
            for g in range(4):
                if k >= cadence[g]:
                    continue
                lo, hi = bounds[g], bounds[g + 1]
                with torch.cuda.stream(streams[g]):
                    a.random_actions_group(g, SEED, out=acts[g], stream=streams[g])
                    a.step_group(g, acts[g], ua[lo:hi], inplace=(rnd % 2 == 1), stream=streams[g])
    for s in streams:
        cur.wait_stream(s)
    torch.cuda.synchronize()
    counts = [6 * c for c in cadence]
    act = torch.empty(n, dtype=torch.int32, device=DEV)
    snaps = {}
    for t in range(1, max(counts) + 1):
        b.random_actions(SEED, act)
        b.step(act, ub, inplace=True)
        for g, c in enumerate(counts):
            if c == t:
                lo, hi = bounds[g], bounds[g + 1]
                snaps[g] = ({k: b.fetch(k)[lo:hi].cpu().numpy().copy() for k in STATE}, ub[lo:hi].cpu().numpy().copy(), _lens(b, lo, hi))
    for g in range(4):
        lo, hi = bounds[g], bounds[g + 1]
        st, rows, lens = snaps[g]
        for k in STATE:
            assert np.array_equal(a.fetch(k)[lo:hi].cpu().numpy(), st[k]), (g, k)
        got = ua[lo:hi].cpu().numpy()
        for i, m in enumerate(lens):
            assert np.array_equal(got[i, :m], rows[i, :m]), (g, i)
    assert_rows_match_oracle(a, ua, 0, n, 0, False, "groups")        # the twin runs the same kernel: the oracle does not


# ---- 5. config-5 size (HBM-scratch route) ------------------------------------------------------------------------------------------
def test_u8_config5_size():
    regions = [generate_region(8400 + i, dims=(256, 256, 12), k_range=(3, 5), net_span=8) for i in range(2)]
    a, b = RegionBatch(regions, device=DEV, auto_reset=True), RegionBatch(regions, device=DEV, auto_reset=True)
    fa, ub = a.alloc_observation(), b.alloc_observation(dtype=torch.uint8)
    for x in (a, b):
        x.reset()
    act = torch.empty(2, dtype=torch.int32, device=DEV)
    for t in range(3):
        a.random_actions(SEED, act)
        a.step(act, fa)
        b.step(act, ub, inplace=(t > 0))
        _assert_state_equal(_state(a), _state(b), ("config5", t))
        _assert_rows_cast(ub, fa, _lens(a), ("config5", t))
    u = b.observation(b.alloc_observation(dtype=torch.uint8))
    _assert_rows_cast(u, a.observation(), _lens(a), "config5 stand-alone")


# ---- 6. scale ---------------------------------------------------------------------------------------------------------------------
def test_u8_4096_slots_against_fp32_twin():
    regions = config_regions(4, 256)
    n = 4096
    a, b = RegionBatch(regions, n_envs=n, device=DEV, auto_reset=True), RegionBatch(regions, n_envs=n, device=DEV, auto_reset=True)
    fa, ub = a.alloc_observation(), b.alloc_observation(dtype=torch.uint8)
    for x in (a, b):
        x.reset(rotate=True)
    act = torch.empty(n, dtype=torch.int32, device=DEV)
    a.random_actions(SEED, act)
    a.step(act, fa)
    b.step(act, ub)
    assert torch.equal(a.fetch("record"), b.fetch("record"))
    assert torch.equal(a.fetch("hash"), b.fetch("hash"))
    lens = _lens(a)
    for e in range(0, n, 61):
        m = lens[e]
        want = hashlib.sha256(fa[e, :m].to(torch.uint8).cpu().numpy().tobytes()).hexdigest()
        assert hashlib.sha256(ub[e, :m].cpu().numpy().tobytes()).hexdigest() == want, e
    del fa


# ---- 7. refusals on a live batch --------------------------------------------------------------------------------------------------
def _raw_step(batch, out_ptr, stride, flags=0, group=-1, act=None):
    L = _lib.lib()
    return L.xr_batch_step_observe_u8(batch._h, group, C.c_void_p(act.data_ptr()), C.c_void_p(out_ptr), stride, flags,
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_u8_refusals_leave_the_batch_untouched():
    regions = [generate_region(8500 + i, dims=(16, 10, 4), k_range=(3, 6), net_span=5) for i in range(4)]
    n = 8
    a, b = _make(regions, n), _make(regions, n)
    for x in (a, b):
        x.reset(rotate=True)
    act = a.random_actions(SEED)
    buf = torch.zeros(n * a.obs_env_stride_u8 + 64, dtype=torch.uint8, device=DEV)
    S = a.obs_env_stride_u8
    base = buf.data_ptr()
    assert base % 16 == 0
    assert _raw_step(a, base + 1, S, act=act) == _lib.XR_ERR_INVALID           # misaligned pointer
    assert _raw_step(a, base, S + 8, act=act) == _lib.XR_ERR_INVALID           # stride not a multiple of 16
    short = ((2 + 7 * a.k_max) * a.n_max // 16) * 16 - 16
    assert _raw_step(a, base, short, act=act) == _lib.XR_ERR_RANGE             # short stride
    assert _raw_step(a, base, S, flags=2, act=act) == _lib.XR_ERR_INVALID      # unknown flags
    assert _raw_step(a, base, S, group=1, act=act) == _lib.XR_ERR_RANGE        # no such group
    L = _lib.lib()
    s0 = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.xr_batch_observation_u8(a._h, C.c_void_p(base + 4), S, 0, n, s0) == _lib.XR_ERR_INVALID
    assert L.xr_batch_observation_u8(a._h, C.c_void_p(base), short, 0, n, s0) == _lib.XR_ERR_RANGE
    torch.cuda.synchronize()
    _assert_state_equal(_state(a), _state(b), "after refusals")
    fa, fb = a.alloc_observation(), b.alloc_observation()
    a.step(act, fa)
    b.step(act, fb)
    _assert_state_equal(_state(a), _state(b), "stepping on")
    # a region with 256 nets: every uint8 call refused (also through Python), the batch keeps stepping in fp32 like its twin
    wide = [dataclasses.replace(regions[0], n_nets=256)] + regions[1:]
    c, d = _make(wide, n), _make(wide, n)
    for x in (c, d):
        x.reset(rotate=True)
    uc = c.alloc_observation(dtype=torch.uint8)
    act = c.random_actions(SEED)
    assert _raw_step(c, uc.data_ptr(), uc.shape[1], act=act) == _lib.XR_ERR_RANGE
    with pytest.raises(_lib.XRouteError):
        c.step(act, uc)
    with pytest.raises(_lib.XRouteError):
        c.observation(uc)
    torch.cuda.synchronize()
    _assert_state_equal(_state(c), _state(d), "256 nets")
    fc, fd = c.alloc_observation(), d.alloc_observation()
    c.step(act, fc)
    d.step(act, fd)
    _assert_state_equal(_state(c), _state(d), "256 nets, stepping on")
    with pytest.raises(ValueError):
        a.step(act, torch.zeros((n, 64), dtype=torch.int16, device=DEV))


# ---- 8. vector env ----------------------------------------------------------------------------------------------------------------
def test_vector_env_u8_equals_fp32_cast():
    from xroute_env_amd.envs.vector_env import XRouteVectorEnv
    regions = [generate_region(8600 + i, dims=(12, 10, 4), k_range=(2, 5), net_span=5) for i in range(6)]
    f = XRouteVectorEnv(regions, n_envs=12, device=DEV, max_route_count=1, groups=2, dict_observation=True)
    u = XRouteVectorEnv(regions, n_envs=12, device=DEV, max_route_count=1, groups=2, dict_observation=True, obs_dtype=torch.uint8)
    assert u.observation_space["grid"].dtype == np.uint8 and f.observation_space["grid"].dtype == np.float32
    assert u.single_observation_space["grid"].dtype == np.uint8
    assert u.observation_space["grid"].shape == (12, u.batch.obs_env_stride_u8)

    def same(of, ou, what):
        assert ou["grid"].dtype == torch.uint8
        assert torch.equal(of["legal_mask"], ou["legal_mask"])
        _assert_rows_cast(ou["grid"], of["grid"], _lens(f.batch, 0, of["grid"].shape[0]), what)

    of, _ = f.reset()
    ou, _ = u.reset()
    same(of, ou, "reset")
    for t in range(8):
        act = f.random_actions(SEED)
        of, rf, df, _ = f.step(act)
        ou, ru, du, _ = u.step(act)
        assert torch.equal(rf, ru) and torch.equal(df, du)
        same(of, ou, ("step", t))
    for t in range(4):
        act = f.random_actions(SEED)
        f.step_async(act)
        u.step_async(act)
        of, rf, _, _ = f.step_wait()
        ou, ru, _, _ = u.step_wait()
        assert torch.equal(rf, ru)
        same(of, ou, ("async", t))
    assert u.observation_dict()["grid"].dtype == torch.uint8


# ---- 9. agents --------------------------------------------------------------------------------------------------------------------
def test_agents_pick_the_same_actions_from_the_u8_grid():
    from xroute_env_amd import agents
    torch.manual_seed(0)
    regions = [generate_region(9300 + i) for i in range(16)]
    dims = regions[0].dims
    batch = RegionBatch(regions, device=DEV, auto_reset=True)
    batch.reset()
    dqn = agents.RepActor().to(DEV).eval()
    ppo = agents.ActorCritic(64).to(DEV).eval()
    fused = {}
    for name, m in (("dqn", dqn), ("ppo", ppo)):
        cache = agents.NetVectorCache(len(regions), batch.k_max, DEV)
        cache.prefill(m.representation_network, [r.n_nets for r in regions], batch.net_planes, dims)
        tower = agents.FusedObstacleTower(m.representation_network, (dims[2], dims[1], dims[0]), DEV)
        assert tower.supported
        fused[name] = dict(cache=cache, ob_tower=tower, actor_head=agents.FusedActorHead(m.actor, DEV), planes_fn=batch.net_planes)
    f, u = batch.alloc_observation(), batch.alloc_observation(dtype=torch.uint8)
    nl = torch.empty(len(regions), dtype=torch.int32, device=DEV)
    reg = torch.empty(len(regions), dtype=torch.int32, device=DEV)
    ids = torch.arange(len(regions), dtype=torch.int64, device=DEV)
    for step in range(5):
        batch.observation(f)
        batch.observation(u)
        batch.fetch("nlegal", nl)
        batch.fetch("region", reg)
        a_f = agents.dqn_actions(dqn, f, nl, dims, region=reg, **fused["dqn"])
        a_u = agents.dqn_actions(dqn, u, nl, dims, region=reg, **fused["dqn"])
        assert torch.equal(a_f, a_u), step
        uni = agents.counter_uniform(7, step, ids)
        p_f, v_f = agents.ppo_actions(ppo, f, nl, dims, uniform=uni, region=reg, **fused["ppo"])
        p_u, v_u = agents.ppo_actions(ppo, u, nl, dims, uniform=uni, region=reg, **fused["ppo"])
        assert torch.equal(p_f, p_u) and torch.equal(v_f, v_u), step
        batch.step(a_f)
