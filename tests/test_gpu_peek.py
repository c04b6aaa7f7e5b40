"""Peek on the MI355X (xr_batch_peek / RegionBatch.peek / XRouteVectorEnv.peek, envs/peek.py): the state every env would be in after a
line of play, as a packed state row, without stepping.  Twin rows (every (row, line) == pack_state of a twin brought to the env's state
and stepped along the line, byte for byte; the record == rollout(policy="stop")); heads (expand_state(rows) == the twin's step_compact
head); illegal entries; row padding; slot reuse; purity; every router variant; refusals; env groups on their own streams; the successor
helpers of envs/peek.py."""
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
SEED = 0x9EE4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAD = _lib.XR_ENV_BAD_ACTION


@pytest.fixture(autouse=True)
def _release_cached_memory():
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _pack(sl=slice(None)):
    from xroute_env_amd.lefdef import load_region_pack
    return load_region_pack(os.path.join(GOLDEN, "ispd18_test1_regions.npz"))[sl]


def _regions():
    """The "mixed" set, 16 x 12 x 5 (N = 15 * 64), 13 x 17 x 4 (N = 884: N % 8 = 4 and N % 64 != 0 — the cut last chunk and the partial
    last occupancy word), 20 x 14 x 6, and one region with more than 64 nets (two legal words)."""
    from tests.helpers import obs_set_regions
    extra = [generate_region(9100 + i, dims=d, k_range=(4, 10), pins=(3, 5), net_span=7) for i, d in enumerate([(16, 12, 5), (13, 17, 4), (20, 14, 6)])]
    wide = generate_region(9400, dims=(23, 15, 5), k_range=(66, 70), net_span=6, pins=(2, 2), aps=(1, 1))
    return obs_set_regions("mixed") + extra + [wide]


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
    for i in range(start, start + steps):
        act = b.random_actions(SEED + 1000 + i)
        b.step(act)
        if history is not None:
            for e, a in enumerate(act.cpu().numpy().tolist()):
                if a:
                    history[e].append(a)


def _line(kind, e, nets, most=None):
    """The nets of one line of env e: kind 0 nothing, 1 one net, 2 two nets (the last, then the first), 3 all of them (rotated by e; at
    most `most`).  A done env gets two entries that nothing may look at."""
    if nets.size == 0:
        return [1, 2] if kind else []
    if kind == 0:
        return []
    if kind == 1:
        return [int(nets[e % nets.size])]
    if kind == 2:
        return [int(nets[-1]), int(nets[0])] if nets.size >= 2 else [int(nets[0])]
    return [int(v) for v in np.roll(nets, e)[:most]]


def _prefix(legal, L, stride, kind_of, most=None):
    """int32 [n, L, stride]: line l of env e is _line(kind_of(e, l), ...) — consecutive lines of an env differ, and so do the same lines
    of consecutive envs: a shadow slot that kept anything of its last task would show."""
    n = legal.shape[0]
    p = np.zeros((n, L, stride), np.int32)
    for e in range(n):
        nets = np.flatnonzero(legal[e]) + 1
        for l in range(L):
            ln = _line(kind_of(e, l), e, nets, most)
            p[e, l, :len(ln)] = ln
    return p


def _until_terminator(cols):
    """[n, stride] entries of one line per env, everything from the first value <= 0 on zeroed (the list ends there)."""
    live = np.cumprod(cols > 0, axis=1).astype(bool)
    return np.where(live, cols, 0).astype(np.int32)


class _Twin:
    """A batch of the same config with auto_reset off, brought to the state of `a` (load_state_dict) and stepped along one line per env:
    what the line's row, head, nlegal and region must equal."""

    def __init__(self, regions, n, **kw):
        self.t = RegionBatch(regions, n_envs=n, device=DEV, **dict(kw, auto_reset=False))
        self.t.reset()
        self.head = self.t.alloc_head()
        self.act = torch.zeros(n, dtype=torch.int32, device=DEV)

    def after(self, sd, cols, region_base=0, row_bytes=None):
        """cols: [n, stride] the line of every env (illegal entries are flagged no-ops of the step: the twin skips them too)."""
        t = self.t
        t.load_state_dict(sd)
        cols = _until_terminator(cols)
        steps = int((cols > 0).sum(1).max()) if cols.size else 0
        for j in range(max(steps, 1)):          # (at least one compact step, of no-ops if need be: the head of the state as it is)
            self.act.copy_(torch.from_numpy(np.ascontiguousarray(cols[:, j])))
            t.step_compact(self.act, self.head)
        return dict(rows=t.pack_state(region_base=region_base, row_bytes=row_bytes).cpu().numpy(), head=self.head.cpu().numpy().copy(),
                    nlegal=t.fetch("nlegal").cpu().numpy(), region=t.fetch("region").cpu().numpy())

    def close(self):
        self.t.close()


def _assert_rows_and_heads(a, res, prefix, twin, sd, regions, what, region_base=0):
    """EVERY (row, line): the row == the twin's pack_state over the bytes peek writes; expand_state(rows) == the twin's compact head over
    the 2 * N floats of the env's region, nlegal and region (+ region_base); no row flagged.  Returns the number of pairs compared."""
    n, L, rb = res["rows"].shape
    need = a.state_row_bytes()
    assert need == 16 + 8 * (a.legal_words + (a.n_max + 63) // 64) and rb >= need
    rows = res["rows"].cpu().numpy()
    head = nl = rg = None
    if region_base == 0:
        head, nl, rg = a.expand_state(res["rows"].reshape(n * L, rb))
        head, nl, rg = head.cpu().numpy().reshape(n, L, -1), nl.cpu().numpy().reshape(n, L), rg.cpu().numpy().reshape(n, L)
        assert (nl >= 0).all() and (rg >= 0).all(), what
    reg = a.fetch("region").cpu().numpy()
    n2 = np.array([2 * regions[int(r)].n_nodes for r in reg])
    in_head = np.arange(2 * a.n_max)[None, :] < n2[:, None]
    for l in range(L):
        tw = twin.after(sd, prefix[:, l], region_base=region_base, row_bytes=rb)
        assert np.array_equal(rows[:, l, :need], tw["rows"][:, :need]), (what, l, np.flatnonzero((rows[:, l, :need] != tw["rows"][:, :need]).any(1)))
        assert np.array_equal(rows[:, l, :4].copy().view(np.int32)[:, 0], reg + region_base), (what, l)
        if head is not None:
            assert np.array_equal(nl[:, l], tw["nlegal"]) and np.array_equal(rg[:, l], tw["region"]) and np.array_equal(tw["region"], reg), (what, l)
            assert np.array_equal(head[:, l].view(np.uint32)[in_head], tw["head"].view(np.uint32)[in_head]), (what, l)
    return n * L


def _assert_record_equals_rollout_stop(a, res, prefix, what, max_plies=0):
    ro = _np(a.rollout(prefix.shape[1], 0, policy="stop", prefix=torch.from_numpy(prefix).to(DEV), max_plies=max_plies))
    got = _np({k: res[k] for k in ("out", "ret", "hash", "order")})
    for k in ("out", "hash", "order"):
        assert np.array_equal(got[k], ro[k]), (what, k)
    assert np.array_equal(got["ret"].view(np.uint64), ro["ret"].view(np.uint64)), (what, "return bits")
    return got


# ---- 1. twin rows and heads ------------------------------------------------------------------------------------------------------
def test_every_row_equals_the_packed_state_of_a_twin_stepped_along_the_line():
    regions = _regions()
    n, L = 2 * len(regions), 4
    a = RegionBatch(regions, n_envs=n, device=DEV, auto_reset=False)
    assert a.legal_words >= 2
    a.reset()
    assert set(a.fetch("region").cpu().numpy().tolist()) == set(range(len(regions)))
    twin = _Twin(regions, n)
    taken = compared = 0
    seen = dict(two=0, empty=0, ends=0, done=0)
    for at in (0, 2, 5):
        _advance(a, at - taken, start=taken)
        taken = at
        legal = _legal_matrix(a)
        nl0 = a.fetch("nlegal").cpu().numpy()
        prefix = _prefix(legal, L, a.k_max + 1, lambda e, l: (e + l) % 4)
        before = _snapshot(a)
        res = a.peek(torch.from_numpy(prefix).to(DEV))
        assert _snapshot(a) == before
        assert tuple(res["rows"].shape) == (n, L, a.state_row_bytes()) and res["rows"].dtype == torch.uint8
        got = _assert_record_equals_rollout_stop(a, res, prefix, at)
        compared += _assert_rows_and_heads(a, res, prefix, twin, a.state_dict(), regions, at)
        plies, left = got["out"][:, :, 4], got["out"][:, :, 5]
        live = nl0 > 0
        assert np.array_equal(plies[live], (_until_terminator(prefix.reshape(n * L, -1)) > 0).sum(1).reshape(n, L)[live])
        assert not got["out"][~live].any() and not got["order"][~live].any()          # a done env: the empty record
        seen["two"] += int((plies >= 2).sum()); seen["empty"] += int((plies[live] == 0).sum())
        seen["ends"] += int(((plies > 0) & (left == 0)).sum()); seen["done"] += int((~live).sum())
    assert compared == 3 * n * L
    assert all(v > 0 for v in seen.values()), seen
    twin.close()


def test_region_base_and_max_plies():
    regions = _regions()
    n, L = 2 * len(regions), 4
    a = RegionBatch(regions, n_envs=n, device=DEV, auto_reset=False)
    a.reset()
    _advance(a, 1)
    twin = _Twin(regions, n)
    prefix = _prefix(_legal_matrix(a), L, a.k_max + 1, lambda e, l: (e + l) % 4)
    res = a.peek(torch.from_numpy(prefix).to(DEV), region_base=5)
    _assert_record_equals_rollout_stop(a, res, prefix, "region_base")
    assert _assert_rows_and_heads(a, res, prefix, twin, a.state_dict(), regions, "region_base", region_base=5) == n * L
    # max_plies = 2: the record is rollout's under the same cap, the rows those of the lines cut to two nets
    cut = a.peek(torch.from_numpy(prefix).to(DEV), max_plies=2)
    got = _assert_record_equals_rollout_stop(a, cut, prefix, "max_plies", max_plies=2)
    assert got["out"][:, :, 4].max() == 2
    short = prefix.copy()
    short[:, :, 2:] = 0
    assert torch.equal(cut["rows"], a.peek(torch.from_numpy(short).to(DEV))["rows"])
    assert _assert_rows_and_heads(a, cut, short, twin, a.state_dict(), regions, "max_plies") == n * L
    twin.close()


def test_no_prefix_peeks_the_current_state():
    regions = _regions()
    n = 2 * len(regions)
    a = RegionBatch(regions, n_envs=n, device=DEV, auto_reset=False)
    a.reset()
    _advance(a, 3)
    res = a.peek(None, n_lines=3)
    want = a.pack_state()
    for l in range(3):
        assert torch.equal(res["rows"][:, l], want), l
    got = _np(res)
    assert not got["out"][:, :, :5].any() and not got["out"][:, :, 6:].any() and not got["order"].any()
    assert np.array_equal(got["out"][:, :, 5], np.repeat(a.fetch("nlegal").cpu().numpy()[:, None], 3, 1))
    assert (got["ret"].view(np.uint64) == 0).all() and np.array_equal(got["hash"], np.repeat(a.fetch("hash").cpu().numpy()[:, None], 3, 1))
    with pytest.raises(ValueError, match="n_lines"):
        a.peek(None)


# ---- 2. illegal entries ----------------------------------------------------------------------------------------------------------
def test_entries_that_are_not_legal_are_skipped_and_flagged_and_the_row_is_the_twins():
    regions = _regions()
    n = 2 * len(regions)
    a = RegionBatch(regions, n_envs=n, device=DEV, auto_reset=False)
    a.reset()
    history = [[] for _ in range(n)]
    _advance(a, 2, history)
    legal = _legal_matrix(a)
    prefix = np.zeros((n, 3, 8), np.int32)
    flagged = np.zeros((n, 3), bool)
    real = np.zeros((n, 3), np.int32)
    for e in range(n):
        nets = (np.flatnonzero(legal[e]) + 1).tolist()
        if not nets:                                                   # a done env: nothing looked at, nothing flagged
            prefix[e, :, :2] = [history[e][0], 1]
            continue
        x, c = nets[0], nets[-1]
        prefix[e, 0, :4] = [x, x, c, x]                                # repeated
        prefix[e, 1, :5] = [history[e][0], x, a.k_max + 7, 70000, c]   # already routed, beyond k_max, beyond every legal word
        prefix[e, 2, :3] = [c, 0, x]                                   # the terminator ends the list: `x` is never seen
        real[e] = [2 if c != x else 1, 2 if c != x else 1, 1]
        flagged[e] = [len(nets) > 1, True, False]                      # (one net left: everything routed after it, the rest is ignored)
    res = a.peek(torch.from_numpy(prefix).to(DEV))
    got = _assert_record_equals_rollout_stop(a, res, prefix, "illegal")
    assert np.array_equal((got["out"][:, :, 3] & BAD) != 0, flagged) and flagged[:, 0].sum() > n // 2
    assert np.array_equal(got["out"][:, :, 4], real)
    twin = _Twin(regions, n)
    assert _assert_rows_and_heads(a, res, prefix, twin, a.state_dict(), regions, "illegal") == n * 3
    twin.close()


# ---- 3. row_bytes above the minimum ----------------------------------------------------------------------------------------------
def test_padding_bytes_of_wider_rows_keep_their_sentinel():
    regions = _regions()
    n, L = 2 * len(regions), 4
    a = RegionBatch(regions, n_envs=n, device=DEV, auto_reset=False)
    a.reset()
    _advance(a, 1)
    need = a.state_row_bytes()
    prefix = torch.from_numpy(_prefix(_legal_matrix(a), L, a.k_max + 1, lambda e, l: (e + l) % 4)).to(DEV)
    tight = a.peek(prefix)["rows"]
    for extra in (8, 40):
        wide = torch.full((n, L, need + extra), 0xAB, dtype=torch.uint8, device=DEV)
        res = a.peek(prefix, rows_out=wide)
        assert res["rows"] is wide
        assert torch.equal(wide[:, :, :need], tight) and bool((wide[:, :, need:] == 0xAB).all()), extra
        assert torch.equal(a.peek(prefix, row_bytes=need + extra)["rows"][:, :, :need], tight)


# ---- 4. slot reuse ---------------------------------------------------------------------------------------------------------------
def test_more_lines_than_resident_workgroups_reuse_the_shadow_slots():
    regions = _regions()
    n = 2 * len(regions)
    a = RegionBatch(regions, n_envs=n, device=DEV, auto_reset=False)
    a.reset()
    _advance(a, 2)
    resident = a.route_occupancy()[0] * torch.cuda.get_device_properties(0).multi_processor_count
    L = min(_lib.XR_PEEK_MAX, resident // n + 3)
    assert n * L > resident
    kinds = 6                                                          # line l repeats line l % 6: six twins cover every line
    kind_of = lambda e, l: (e + l % kinds) % 4
    prefix = _prefix(_legal_matrix(a), L, 4, kind_of, most=3)
    res = a.peek(torch.from_numpy(prefix).to(DEV))
    _assert_record_equals_rollout_stop(a, res, prefix, "reuse")
    twin = _Twin(regions, n)
    first = {k: res[k][:, :kinds].contiguous() for k in res}
    assert _assert_rows_and_heads(a, first, prefix[:, :kinds], twin, a.state_dict(), regions, "reuse") == n * kinds
    for l in range(kinds, L):                                          # every other row against the checked row of the same line
        assert np.array_equal(prefix[:, l], prefix[:, l % kinds])
        assert torch.equal(res["rows"][:, l], res["rows"][:, l % kinds]), l
    twin.close()


# ---- 5. purity -------------------------------------------------------------------------------------------------------------------
def test_peek_leaves_every_fetchable_array_byte_identical():
    regions = _regions()
    n = 2 * len(regions)
    b = RegionBatch(regions, n_envs=n, device=DEV, auto_reset=True, max_route_count=1)
    b.reset()
    act = torch.empty(n, dtype=torch.int32, device=DEV)
    for step in range(8):
        before = _snapshot(b)
        b.peek(torch.from_numpy(_prefix(_legal_matrix(b), 4, 4, lambda e, l: (e + l) % 4, most=3)).to(DEV))
        b.peek(None, n_lines=2)
        b.peek(torch.full((n, 1, 2), 1 + step, dtype=torch.int32, device=DEV), max_plies=1, region_base=3)
        after = _snapshot(b)
        for k in before:
            assert before[k] == after[k], (step, k)
        b.step(b.random_actions(SEED + step, act))


@pytest.mark.parametrize("mode", ["inplace", "inplace_u8"])
def test_a_batch_that_peeks_before_every_step_equals_its_twin_that_never_does(mode):
    regions = _regions()
    n = 2 * len(regions)
    kw = dict(n_envs=n, device=DEV, auto_reset=True, max_route_count=1)
    a, t = RegionBatch(regions, **kw), RegionBatch(regions, **kw)
    a.reset(); t.reset()
    dt = torch.uint8 if mode == "inplace_u8" else torch.float32
    obs_a, obs_t = a.alloc_observation(dtype=dt).zero_(), t.alloc_observation(dtype=dt).zero_()
    a.observation(obs_a); t.observation(obs_t)
    act = torch.empty(n, dtype=torch.int32, device=DEV)
    for step in range(20):
        a.peek(torch.from_numpy(_prefix(_legal_matrix(a), 2, 3, lambda e, l: 1 + (e + l) % 2)).to(DEV))
        a.random_actions(SEED + step, act)
        a.step(act, obs_a, inplace=True)
        t.step(act, obs_t, inplace=True)
        for k in ("hash", "record", "owner", "legal", "region", "replay", "env_steps", "steps", "path", "path_len", "sweeps"):
            assert a.fetch(k).cpu().numpy().tobytes() == t.fetch(k).cpu().numpy().tobytes(), (step, k)
        info = a.observe_info()
        assert info["form"] == 3 and info["inplace"], (step, info)          # the in-place path survived the peek
        assert torch.equal(obs_a, obs_t), step


# ---- 6. variants -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["auto", "sweep", "dial", "dial_r2", "v2_guides"])
def test_peek_under_every_router_variant(variant):
    if variant == "v2_guides":
        regions = _pack(slice(5, 200, 13))[:12]
        assert all(r.guide_off is not None and r.guide_off[-1] > 0 for r in regions)
        kw = dict(guide_cost=1000, guide_margin=1, maze_end_iter=3)
    else:
        regions = [generate_region(3000 + i) for i in range(12)]
        kw = dict(router={"auto": 0, "sweep": 1, "dial": 2, "dial_r2": 3}[variant], dial_mult=0 if variant != "dial" else 5)
    n, L = 2 * len(regions), 4
    a = RegionBatch(regions, n_envs=n, device=DEV, auto_reset=False, **kw)
    a.reset()
    twin = _Twin(regions, n, **kw)
    taken = compared = 0
    for at in (0, 3):
        _advance(a, at - taken, start=taken)
        taken = at
        prefix = _prefix(_legal_matrix(a), L, 5, lambda e, l: (e + l) % 4, most=4)
        res = a.peek(torch.from_numpy(prefix).to(DEV))
        _assert_record_equals_rollout_stop(a, res, prefix, (variant, at))
        compared += _assert_rows_and_heads(a, res, prefix, twin, a.state_dict(), regions, (variant, at))
    assert compared == 2 * n * L
    twin.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(force_scratch_field=True), dict(stream_per_region=True)])
def test_peek_refuses_the_scratch_forms_and_leaves_the_batch_untouched(kw):
    regions = [generate_region(3000 + i, dims=(12, 10, 4), k_range=(3, 6)) for i in range(4)]
    b = RegionBatch(regions, device=DEV, **kw)
    b.reset()
    b.step(b.random_actions(SEED))
    before = _snapshot(b)
    with pytest.raises(_lib.XRouteError) as ei:
        b.peek(None, n_lines=2)
    assert ei.value.code == _lib.XR_ERR_RANGE
    assert _snapshot(b) == before
    b.step(b.random_actions(SEED + 1))            # still usable


# ---- 8. groups -------------------------------------------------------------------------------------------------------------------
def test_groups_peek_concurrently_on_their_own_streams_and_equal_the_whole_batch_rows():
    from xroute_env_amd.envs.vector_env import XRouteVectorEnv
    regions = _regions()
    n, L = 2 * len(regions), 4
    env = XRouteVectorEnv(regions, n_envs=n, device=DEV, max_route_count=1, groups=4, with_observation=False)
    env.reset()
    a = env.batch
    for i in range(2):
        env.step(a.random_actions(SEED + i))
    prefix = torch.from_numpy(_prefix(_legal_matrix(a), L, a.k_max + 1, lambda e, l: (e + l) % 4)).to(DEV)
    whole = env.peek(prefix)
    torch.cuda.synchronize()
    parts = []
    for g in range(4):                                                 # four launches in flight, one per group stream
        lo, hi = a.group_bounds(g)
        parts.append(env.peek(prefix[lo:hi].contiguous(), group=g))
    env.step_wait()
    torch.cuda.synchronize()
    for g, res in enumerate(parts):
        lo, hi = a.group_bounds(g)
        assert tuple(res["rows"].shape) == (hi - lo, L, a.state_row_bytes())
        for k in ("rows", "out", "hash", "order"):
            assert torch.equal(res[k], whole[k][lo:hi]), (g, k)
        assert torch.equal(res["ret"].view(torch.int64), whole["ret"][lo:hi].view(torch.int64)), g
    # the batch's own interface, on streams of the caller
    streams = [torch.cuda.Stream() for _ in range(4)]
    cur = torch.cuda.current_stream()
    parts = []
    for g, s in enumerate(streams):
        lo, hi = a.group_bounds(g)
        s.wait_stream(cur)
        with torch.cuda.stream(s):
            parts.append(a.peek(prefix[lo:hi].contiguous(), group=g, stream=s))
    for s in streams:
        cur.wait_stream(s)
    torch.cuda.synchronize()
    for g, res in enumerate(parts):
        lo, hi = a.group_bounds(g)
        assert torch.equal(res["rows"], whole["rows"][lo:hi]), g


# ---- 9. envs/peek.py -------------------------------------------------------------------------------------------------------------
def test_successor_prefix_lists_every_legal_net_in_ascending_order():
    from xroute_env_amd.envs.peek import successor_prefix
    regions = _regions()
    n = 2 * len(regions)
    a = RegionBatch(regions, n_envs=n, device=DEV, auto_reset=False)
    a.set_groups(3)
    a.reset()
    _advance(a, 2)
    legal = _legal_matrix(a)
    want = np.zeros((n, a.k_max, 1), np.int32)
    for e in range(n):
        nets = np.flatnonzero(legal[e]) + 1
        want[e, :nets.size, 0] = nets
    got = successor_prefix(a)
    assert got.dtype == torch.int32 and got.is_contiguous() and np.array_equal(got.cpu().numpy(), want)
    lo, hi = a.group_bounds(1)
    assert np.array_equal(successor_prefix(a, group=1).cpu().numpy(), want[lo:hi])
    assert want.max() > 64                                             # nets of the second legal word


def _model():
    from xroute_env_amd.agents import ActorCritic
    torch.manual_seed(7)
    return ActorCritic(device=DEV).to(DEV).eval()


@pytest.mark.parametrize("tower", ["fused", "module"])
def test_successor_values_equal_the_critic_on_the_twins_compact_heads(tower):
    from xroute_env_amd.agents import FusedObstacleTower
    from xroute_env_amd.envs import peek as pk
    # two grid shapes: 24 x 40 x 9 (the grid the fused tower is built for here) and 22 x 30 x 9 (no tower given: the module's convolutions)
    regions = [generate_region(3000 + i, k_range=(3, 5), **({} if i % 2 == 0 else dict(dims=(22, 30, 9)))) for i in range(6)]
    n, chunk = 12, 4
    a = RegionBatch(regions, n_envs=n, device=DEV, auto_reset=False)
    a.reset()
    _advance(a, 1)
    model = _model()
    X, Y, Z = (int(v) for v in regions[0].dims)
    towers = None
    if tower == "fused":
        towers = {(X, Y, Z): FusedObstacleTower(model.representation_network, (Z, Y, X), DEV)}
        assert towers[(X, Y, Z)].supported
    groups = pk.shape_groups(a)
    assert [d for d, _ in groups] == [(22, 30, 9), (24, 40, 9)] and sorted(torch.cat([i for _, i in groups]).tolist()) == list(range(n))
    before = _snapshot(a)
    values, rewards = pk.successor_values(model, a, towers, chunk=chunk, return_rewards=True, groups=groups)
    assert _snapshot(a) == before
    K = a.k_max
    assert values.dtype == torch.float32 and tuple(values.shape) == (n, K) and rewards.dtype == torch.float64
    assert torch.equal(values, pk.successor_values(model, a, towers, chunk=chunk))
    # the same heads from twins: candidate c of every env stepped by step_compact, then the same functions on the same pieces
    legal = _legal_matrix(a)
    nets = pk.successor_prefix(a)[:, :, 0]
    twin = _Twin(regions, n)
    sd = a.state_dict()
    heads = torch.zeros((n, K, 2 * a.n_max), dtype=torch.float32, device=DEV)
    for c in range(K):
        heads[:, c] = torch.from_numpy(twin.after(sd, nets[:, c:c + 1].cpu().numpy())["head"]).to(DEV)
    want = torch.full((n, K), float("-inf"), dtype=torch.float32, device=DEV)
    for dims, idx in groups:
        for lo in range(0, idx.numel(), chunk):
            sel = idx[lo:lo + chunk]
            v = pk.state_values(model, heads.index_select(0, sel).reshape(sel.numel() * K, -1), dims, towers).reshape(sel.numel(), K)
            want.index_copy_(0, sel, pk._by_net(v, nets.index_select(0, sel), float("-inf")))
    assert torch.equal(values, want)
    assert np.array_equal(torch.isfinite(values).cpu().numpy(), legal) and legal.sum() > n
    _, look = a.lookahead()
    assert torch.equal((rewards + 0.0).view(torch.int64), (0.0 + look).view(torch.int64))          # the step reward of every candidate
    # value_actions: the first maximum of reward + value; 0 for a done env
    act = pk.value_actions(model, a, towers, chunk=chunk).cpu().numpy()
    score = (rewards + values.to(torch.float64)).cpu().numpy()
    for e in range(n):
        assert act[e] == (int(np.argmax(score[e])) + 1 if legal[e].any() else 0), e
    twin.close()


def test_value_actions_ties_and_done_envs_and_a_tree_search_under_the_value_prior():
    from xroute_env_amd.envs import peek as pk
    from xroute_env_amd.envs.vector_env import XRouteVectorEnv
    regions = [generate_region(3000 + i, k_range=(2, 2) if i % 2 else (5, 5)) for i in range(6)]
    n = 12
    a = RegionBatch(regions, n_envs=n, device=DEV, auto_reset=False)
    a.reset()
    _advance(a, 3)                                                     # regions of two and three nets are done by now
    legal = _legal_matrix(a)
    assert (~legal.any(1)).any() and legal.any(1).any()
    model = _model()
    with torch.no_grad():
        for p in model.critic.parameters():                           # a constant critic: reward + value ties wherever the rewards tie
            p.zero_()
    values, rewards = pk.successor_values(model, a, return_rewards=True)
    assert bool((values[torch.isfinite(values)] == 0).all())
    act = pk.value_actions(model, a).cpu().numpy()
    r = rewards.cpu().numpy()
    for e in range(n):
        assert act[e] == (int(np.flatnonzero(r[e] == r[e].max())[0]) + 1 if legal[e].any() else 0), e
    tie = torch.full((2, 4), float("-inf"), dtype=torch.float64)
    tie[0, 1] = tie[0, 3] = -2.0
    assert pk.pick_best(tie).tolist() == [2, 0]
    prior, weights = pk.value_prior(values, rewards, 0.5)
    assert np.array_equal((prior > 0).cpu().numpy(), legal) and np.array_equal((weights > 0).cpu().numpy(), legal)
    assert np.allclose(prior.sum(1).cpu().numpy(), legal.any(1).astype(np.float32), atol=1e-5)
    before = _snapshot(a)
    res = a.tree_search(4, 4, seed=SEED, prior=prior, sim_weights=weights)
    assert _snapshot(a) == before
    best = XRouteVectorEnv._most_visited(res).cpu().numpy()
    for e in range(n):
        assert (best[e] > 0 and legal[e, best[e] - 1]) if legal[e].any() else best[e] == 0, (e, best[e])
