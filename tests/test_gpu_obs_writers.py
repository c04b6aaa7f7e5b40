"""Every observation writer against the oracle at every alignment class (tests/helpers.py: OBS_SHAPE_SETS).

Each test drives one writer form (stand-alone, the fp32 step forms, the uint8 step, env groups; full write and in place; the
allocator's row stride and odd ones) over one row of the shape table, through auto-resets with region rotation and rejected actions,
and compares every row with oracle.build_observation of the state fetched from the batch under test — never with a twin running the
same kernel.  What a step may write behind an env's (2+7K)N values: include/xroute_hip.h says "bytes past (2+7K)*N are never
written" for the uint8 calls and nothing for fp32, where the stand-alone and split-form tests already require the same; every
full-write form is held to it (helpers.assert_rows_match_oracle)."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from tests.helpers import OBS_SETS, SENTINEL_F32, SENTINEL_U8, assert_rows_match_oracle, obs_set_regions
from xroute_env_amd import _lib
from xroute_env_amd.batch import RegionBatch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x0B5E
F32, U8 = torch.float32, torch.uint8
BIG = ("many_nets", "exactly_255")          # episodes of 200+ steps, rows of megabytes: fewer slots, route-only steps up to the episode's end first


@pytest.fixture(autouse=True)
def _release_cached_memory():
    """Sentinel checks read whole rows: no test may inherit another's bytes from the caching allocator."""
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _shape(name):
    """(slots, observed steps, group bounds) of a set: more slots than regions, so that rotation changes a slot's region."""
    return (7, 6, [0, 1, 4, 7]) if name in BIG else (17, 8, [0, 1, 7, 13, 17])


def _batch(name, **kw):
    regions = obs_set_regions(name)
    return RegionBatch(regions, n_envs=_shape(name)[0], device=DEV, auto_reset=True, max_route_count=1, **kw)


def _sentinel(dtype):
    return SENTINEL_U8 if dtype == U8 else SENTINEL_F32


def _buffer(batch, dtype, extra=0, rows=None):
    stride = (batch.obs_env_stride_u8 if dtype == U8 else batch.obs_env_stride) + extra
    return torch.full((batch.n_envs if rows is None else rows, stride), _sentinel(dtype), dtype=dtype, device=DEV)


def _start(batch, name):
    """reset(rotate) and, for the sets with long episodes, route-only steps until the first slots are two nets from their end: the
    observed steps then cross auto-resets and region changes in every set."""
    batch.reset(rotate=True)
    act = torch.empty(batch.n_envs, dtype=torch.int32, device=DEV)
    if name in BIG:
        for t in range(min(r.n_nets for r in batch.regions if r.n_nets > 100) - 2):
            batch.random_actions(SEED + t, act)
            batch.step(act)
    return act


def _reject_some(act):
    act[::3] = 0                     # action 0 and an id beyond every region's nets: flagged no-ops, the observation is still written
    act[1::3] = 9999


# ---- stand-alone writers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, U8], ids=["f32", "u8"])
@pytest.mark.parametrize("name", OBS_SETS)
def test_observation_matches_oracle(name, dtype):
    batch = _batch(name)
    n = batch.n_envs
    act = _start(batch, name)
    seen = set()
    for t in range(4):
        for extra in (0, 48):
            buf = _buffer(batch, dtype, extra)
            batch.observation(buf)
            seen.add(tuple(assert_rows_match_oracle(batch, buf, 0, n, _sentinel(dtype), True, (name, "observation", t, extra))))
        sub = _buffer(batch, dtype, 16, rows=3)
        batch.observation(sub, env_lo=2, env_hi=5)
        assert_rows_match_oracle(batch, sub, 2, 5, _sentinel(dtype), True, (name, "observation[2:5]", t))
        for k in range(2):
            batch.random_actions(SEED + 500 + 2 * t + k, act)
            batch.step(act)
    assert len(seen) > 1                                     # slots finished, re-initialised and rotated on the way


# ---- whole-batch step forms -----------------------------------------------------------------------------------------------------------
# id -> (dtype, obs_mode, in place, extra row stride in elements, the form observe_info() must report)
STEP_FORMS = {
    "f32_fused": (F32, 1, False, 0, 1),
    "f32_split": (F32, 2, False, 0, 2),
    "f32_queue": (F32, 3, False, 0, 3),
    "f32_queue_inplace": (F32, 0, True, 0, 3),
    "f32_stride_plus4": (F32, 0, False, 4, 3),
    "f32_stride_plus4_inplace": (F32, 0, True, 4, 3),
    "f32_stride_plus1": (F32, 0, False, 1, 1),               # rows that are not 16-byte aligned: the header sends the call to XR_OBS_FUSED
    "u8_full": (U8, 0, False, 0, 3),
    "u8_inplace": (U8, 0, True, 0, 3),
    "u8_stride_plus16": (U8, 0, False, 16, 3),               # legal through the C ABI; the unit starts' distance to their 128-byte line
    "u8_stride_plus16_inplace": (U8, 0, True, 16, 3),        # then differs from env to env
    "u8_stride_plus48": (U8, 0, False, 48, 3),
    "u8_stride_plus48_inplace": (U8, 0, True, 48, 3),
}


@pytest.mark.parametrize("form", STEP_FORMS)
@pytest.mark.parametrize("name", OBS_SETS)
def test_step_matches_oracle(name, form):
    dtype, obs_mode, inplace, extra, want_form = STEP_FORMS[form]
    batch = _batch(name, obs_mode=obs_mode)
    n, steps, _ = _shape(name)
    sent = _sentinel(dtype)
    buf = _buffer(batch, dtype, extra)
    assert buf.data_ptr() % 16 == 0
    act = _start(batch, name)
    if inplace:                                              # the buffer holds the observation before the first step
        batch.observation(buf)
        assert_rows_match_oracle(batch, buf, 0, n, sent, True, (name, form, "primed"))
    seen, rejected = set(), 0
    for t in range(steps):
        batch.random_actions(SEED + 1000 + t, act)
        if t in (1, 2):                                      # (twice: a slot that re-initialises in one of the steps is live in the other)
            _reject_some(act)
        if not inplace:
            buf.fill_(sent)
        batch.step(act, buf, inplace=inplace)
        info = batch.observe_info()
        assert info["form"] == want_form and info["inplace"] == inplace, (name, form, t, info)    # no silent fallback hides the writer
        if t in (1, 2):
            rejected += int((batch.fetch("status") & _lib.XR_ENV_BAD_ACTION).ne(0).sum())
        seen.add(tuple(assert_rows_match_oracle(batch, buf, 0, n, sent, not inplace, (name, form, t))))
    assert rejected > 0
    assert len(seen) > 1


# ---- env groups -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inplace", [False, True], ids=["full", "inplace"])
@pytest.mark.parametrize("dtype", [F32, U8], ids=["f32", "u8"])
@pytest.mark.parametrize("name", OBS_SETS)
def test_group_steps_match_oracle(name, dtype, inplace):
    """Every group on its own stream with its own cadence; after every round all rows against the oracle."""
    batch = _batch(name)
    n, steps, bounds = _shape(name)
    G = len(bounds) - 1
    batch.set_groups(bounds)
    sent = _sentinel(dtype)
    buf = _buffer(batch, dtype)
    _start(batch, name)
    if inplace:
        batch.observation(buf)                               # validates every group's rows
        assert_rows_match_oracle(batch, buf, 0, n, sent, True, (name, "groups", "primed"))
    cur = torch.cuda.current_stream()
    streams = [torch.cuda.Stream() for _ in range(G)]
    acts = []
    for g, s in enumerate(streams):
        s.wait_stream(cur)
        with torch.cuda.stream(s):
            acts.append(torch.empty(bounds[g + 1] - bounds[g], dtype=torch.int32, device=DEV))
    cadence = [1, 2, 3, 2][:G]
    seen, rejected = set(), 0
    for rnd in range(max(3, steps // 3)):
        for k in range(max(cadence)):
            seed = SEED + 2000 + rnd * max(cadence) + k      # another seed every step, as in the whole-batch test
            for g in range(G):
                if k >= cadence[g]:
                    continue
                lo, hi = bounds[g], bounds[g + 1]
                with torch.cuda.stream(streams[g]):
                    batch.random_actions_group(g, seed, out=acts[g], stream=streams[g])
                    if rnd in (1, 2) and k == cadence[g] - 1:
                        _reject_some(acts[g])
                    if not inplace:
                        buf[lo:hi].fill_(sent)
                    batch.step_group(g, acts[g], buf[lo:hi], inplace=inplace, stream=streams[g])
                info = batch.observe_info()
                assert info["form"] == 3 and info["inplace"] == inplace, (name, g, rnd, k, info)
        for s in streams:
            cur.wait_stream(s)
        torch.cuda.synchronize()
        if rnd in (1, 2):
            rejected += int((batch.fetch("status") & _lib.XR_ENV_BAD_ACTION).ne(0).sum())
        seen.add(tuple(assert_rows_match_oracle(batch, buf, 0, n, sent, not inplace, (name, "groups", rnd))))
    assert rejected > 0
    assert len(seen) > 1


# ---- assign + reset, then in place: a full write -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, U8], ids=["f32", "u8"])
def test_inplace_after_assign_and_reset_is_a_full_write(dtype):
    """xr_batch_assign changes which region a slot plays without touching the in-place bookkeeping; the reset that must follow it
    (include/xroute_hip.h: the assignment takes effect at the next reset) drops it: the next in-place step writes everything."""
    batch = _batch("mixed")
    n = batch.n_envs
    sent = _sentinel(dtype)
    buf = _buffer(batch, dtype)
    act = _start(batch, "mixed")
    batch.observation(buf)
    batch.random_actions(SEED, act)
    batch.step(act, buf, inplace=True)
    assert batch.observe_info()["inplace"]
    before = batch.fetch("region").cpu().tolist()
    batch.assign([(r + 3) % len(batch.regions) for r in before])
    batch.reset()
    after = batch.fetch("region").cpu().tolist()
    assert after == [(r + 3) % len(batch.regions) for r in before]
    buf.fill_(sent)                                          # whatever the buffer held is gone: only a full write can pass
    batch.random_actions(SEED + 1, act)
    batch.step(act, buf, inplace=True)
    info = batch.observe_info()
    assert info["form"] == 3 and not info["inplace"]
    assert_rows_match_oracle(batch, buf, 0, n, sent, True, ("assign", "full"))
    batch.random_actions(SEED + 2, act)
    batch.step(act, buf, inplace=True)
    assert batch.observe_info()["inplace"]
    assert_rows_match_oracle(batch, buf, 0, n, sent, False, ("assign", "in place again"))


# ---- exactly 255 nets is accepted -----------------------------------------------------------------------------------------------------
def test_u8_accepts_exactly_255_nets():
    batch = _batch("exactly_255")
    assert batch.k_max == 255 and batch.legal_words == 4
    n = batch.n_envs
    batch.reset()
    buf = _buffer(batch, U8)
    batch.observation(buf)
    reg = batch.fetch("region").cpu().tolist()
    N = batch.regions[0].n_nodes
    rows = buf.cpu().numpy()
    e = reg.index(0)
    assert np.array_equal(rows[e, N:N + 255], np.arange(1, 256, dtype=np.uint8))       # plane 1: every id up to 255, as a byte
    assert_rows_match_oracle(batch, buf, 0, n, SENTINEL_U8, True, "255 nets, stand-alone")
    act = batch.random_actions(SEED)
    buf.fill_(SENTINEL_U8)
    rc = _lib.lib().xr_batch_step_observe_u8(batch._h, -1, C.c_void_p(act.data_ptr()), C.c_void_p(buf.data_ptr()), buf.shape[1], 0,
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.XR_OK
    assert_rows_match_oracle(batch, buf, 0, n, SENTINEL_U8, True, "255 nets, step")


# ---- consumers of ids of 128 and more -------------------------------------------------------------------------------------------------
def test_vector_env_and_agents_take_large_ids_from_the_u8_grid():
    from xroute_env_amd import agents
    from xroute_env_amd.envs.vector_env import XRouteVectorEnv
    regions = obs_set_regions("many_nets")
    dims = regions[0].dims
    N = regions[0].n_nodes
    n = 6
    f = XRouteVectorEnv(regions, n_envs=n, device=DEV, max_route_count=1, dict_observation=True)
    u = XRouteVectorEnv(regions, n_envs=n, device=DEV, max_route_count=1, dict_observation=True, obs_dtype=U8)
    torch.manual_seed(0)
    dqn = agents.RepActor().to(DEV).eval()
    ppo = agents.ActorCritic(64).to(DEV).eval()
    ids = torch.arange(n, dtype=torch.int64, device=DEV)

    def same(of, ou, what):
        gf, gu = of["grid"], ou["grid"]
        assert gu.dtype == U8 and gf.dtype == F32
        nl = f.batch.fetch("nlegal")
        assert torch.equal(nl, u.batch.fetch("nlegal")) and torch.equal(of["legal_mask"], ou["legal_mask"])
        reg = f.batch.fetch("region").cpu().tolist()
        legal = u.batch.legal_sets()
        for e in range(n):
            m = (2 + 7 * int(nl[e])) * N
            assert torch.equal(gu[e, :m], gf[e, :m].to(U8)) and torch.equal(gu[e, :m].to(F32), gf[e, :m]), (what, e)
            want = sorted(legal[e])
            assert max(want) >= 128                           # plane 1 holds ids a signed byte would not
            assert gu[e, N:N + len(want)].cpu().tolist() == want and gf[e, N:N + len(want)].cpu().tolist() == want, (what, e)
            assert regions[reg[e]].n_nets > 128
        # the agents' framework path (this shape is beyond the fused towers' prefilled caches: no fused kernels handed in) widens the
        # byte grid itself and must choose what it chooses from the fp32 grid
        a_f = agents.dqn_actions(dqn, gf, nl, dims)
        a_u = agents.dqn_actions(dqn, gu, nl, dims)
        assert torch.equal(a_f, a_u), what
        uni = agents.counter_uniform(7, 0, ids)
        p_f, v_f = agents.ppo_actions(ppo, gf, nl, dims, uniform=uni)
        p_u, v_u = agents.ppo_actions(ppo, gu, nl, dims, uniform=uni)
        assert torch.equal(p_f, p_u) and torch.equal(v_f, v_u), what
        return a_f

    of, _ = f.reset()
    ou, _ = u.reset()
    act = same(of, ou, "reset")
    for t in range(4):
        of, rf, df, _ = f.step(act)
        ou, ru, du, _ = u.step(act)
        assert torch.equal(rf, ru) and torch.equal(df, du)
        act = same(of, ou, ("step", t))
        if t == 1:
            act = f.random_actions(SEED)                     # whatever the untrained nets prefer, ids of 128 and more get routed too
