"""The fused actor head (csrc/xr_agent.hip: `xr_actor_kernel<PRE>` behind `xr_agent_actor` / `xr_agent_actor_sample`, wrapped by agents.FusedActorHead) over
every case it accepts, against an fp64 copy of the module on the CPU (tests/actor_shapes.py: weights, inputs, references, the tolerance and where it comes
from).  Called through the C ABI, so that both forms of the kernel — `pre`: cache_pre_dev = vec @ W1^T[64:128] as FusedActorHead computes it, `vec`:
cache_pre_dev = NULL — and both entry points are reached.  Every output lies in the middle of a larger tensor of sentinels: guard rows before and behind
the logits, guard elements around the actions, checked after every call.  Every assertion on a logit carries the measured error (table: LAB_NOTES.md)."""
import copy
import ctypes as C
import functools

import pytest
import torch

from tests import actor_shapes as acs
from tests import tower_shapes as ts
from xroute_env_amd import agents, _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 2                                       # guard rows of kcap logits before and behind, and 8 * GUARD guard actions on either side
SENT_L, SENT_A = 12345.0, -77
XR_OK, XR_ERR_INVALID, XR_ERR_RANGE = 0, -1, -5
RUNS = [(c, f) for c in acs.CASES if c.B > 0 for f in c.forms]
_rid = lambda v: v.name if isinstance(v, acs.Case) else str(v)


@functools.lru_cache(maxsize=None)
def _packed(weights: str) -> torch.Tensor:
    """The kernel's weight block as agents.FusedActorHead packs it (transposed layers), on the device"""
    return agents.FusedActorHead(copy.deepcopy(acs.make_actor(weights)).to(DEV), DEV).weights


def _some(t: torch.Tensor) -> torch.Tensor:
    """`t` on the device; one row of zeros for a batch of no env (the kernel is not launched, the pointers must still be non-null)"""
    return (t if t.shape[0] else torch.zeros((1,) + tuple(t.shape[1:]), dtype=t.dtype)).to(DEV).contiguous()


def _pre(vec_dev: torch.Tensor, weights: str) -> torch.Tensor:
    return (vec_dev @ _packed(weights)[64 * 128: 128 * 128].view(64, 128)).contiguous()


def _call(m, weights, form, *, rows=None, sample=None, want_logits=True, plain=False, pre=None, **over):
    """One call of the ABI on the made case `m` (`rows`: these envs only).  `sample` = s0: xr_agent_actor_sample with m.env_ids; `plain`: xr_agent_actor.
    `over`: arguments replaced (kcap, head_stride, cache_kmax, n_envs, action = 0 for a NULL pointer).  Returns (status, logits fp32 [B, kcap] or None, actions
    int32 [B]) on the CPU, after the guards around both outputs were found intact; `whole`: the whole guarded tensors instead."""
    c = m.case
    sel = torch.arange(c.B) if rows is None else torch.as_tensor(rows, dtype=torch.int64)
    B = int(sel.numel())
    kcap = over.get("kcap", c.kcap)
    state, head = _some(m.state[sel]), _some(m.head[sel])
    nlegal, region = _some(m.nlegal[sel]), _some(m.region[sel])
    vec = m.vec.to(DEV).contiguous()
    if form == "pre" and pre is None:
        pre = _pre(vec, weights)
    w = _packed(weights)
    big = torch.full((GUARD + max(B, 1) + GUARD, kcap), SENT_L, dtype=torch.float32, device=DEV)
    abuf = torch.full((8 * GUARD + max(B, 1) + 8 * GUARD,), SENT_A, dtype=torch.int32, device=DEV)
    lp = big.data_ptr() + 4 * GUARD * kcap if want_logits else 0
    ap = abuf.data_ptr() + 4 * 8 * GUARD if over.get("action", 1) else 0
    L = _lib.lib()
    with torch.cuda.device(DEV):
        stream = torch.cuda.current_stream(DEV).cuda_stream
        args = [C.c_void_p(state.data_ptr()), C.c_void_p(head.data_ptr()), C.c_int64(over.get("head_stride", head.stride(0))), int(c.ids_off),
                C.c_void_p(nlegal.data_ptr()), C.c_void_p(region.data_ptr()), C.c_void_p(vec.data_ptr()), C.c_void_p(pre.data_ptr() if form == "pre" else 0),
                int(over.get("cache_kmax", c.cache_kmax)), C.c_void_p(w.data_ptr()), int(over.get("n_envs", B)), int(kcap), C.c_void_p(lp), C.c_void_p(ap)]
        if plain:
            assert sample is None
            rc = L.xr_agent_actor(*args, C.c_void_p(stream))
        else:
            ids = m.env_ids[sel].to(DEV).contiguous() if sample is not None else None
            rc = L.xr_agent_actor_sample(*args, C.c_void_p(ids.data_ptr() if ids is not None else 0), C.c_uint64(sample or 0), C.c_void_p(stream))
        torch.cuda.synchronize(DEV)
    big, abuf = big.cpu(), abuf.cpu()
    n = B if rc == XR_OK and over.get("n_envs", B) > 0 else 0                 # rows the call may have written
    lg, act = big[GUARD: GUARD + n], abuf[8 * GUARD: 8 * GUARD + n]
    assert bool((big[:GUARD] == SENT_L).all()) and bool((big[GUARD + n:] == SENT_L).all()), (c.name, form, "a guard row of the logits was written")
    assert bool((abuf[:8 * GUARD] == SENT_A).all()) and bool((abuf[8 * GUARD + n:] == SENT_A).all()), (c.name, form, "a guard element of the actions was written")
    if not want_logits:
        assert bool((big == SENT_L).all())
    return rc, (lg if want_logits else None), act


def _check_logits(m, weights, form, lg, what):
    """Finite exactly at k < min(nlegal, kcap) (no NaN: the poison was not read), -inf behind; within TOL of fp64.  Returns the largest error."""
    ref = acs.logits64(m, weights)
    worst, where = 0.0, None
    for e, r in enumerate(ref):
        n = r.numel()
        assert bool(torch.isfinite(lg[e, :n]).all()), (what, e, "a logit of a legal pair is not finite (poison read?)", lg[e, :n][~torch.isfinite(lg[e, :n])][:4])
        assert bool((lg[e, n:] == float("-inf")).all()), (what, e, "not -inf behind the env's nets")
        if n:
            err = (lg[e, :n].double() - r).abs()
            if float(err.max()) > worst:
                worst, where = float(err.max()), (e, int(err.argmax()))
    print(f"ACTOR_ERR {what} {worst:.2e}")                     # (pytest -s: the table of LAB_NOTES.md)
    assert worst <= acs.TOL[weights], (what, worst, where, acs.TOL[weights])
    return ref


# ---- 1. the greedy path ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", acs.WEIGHT_SETS)
@pytest.mark.parametrize("case,form", RUNS, ids=_rid)
def test_actor_greedy_sweep(case, form, weights):
    """One case of acs.CASES in one form: logits finite exactly where an env has nets and within TOL[weights] of fp64, the fp64 arg-max id as the action of EVERY
    env (0 without nets; the host test holds the top-two distance), the same bits twice, the same actions without a logits buffer, the same bits from
    xr_agent_actor, and a sub-batch (rows 1, 4, 7, ...) gives the rows of the whole batch."""
    what = f"{case.name} {weights} {form}"
    m = acs.make_case(case)
    rc, lg, act = _call(m, weights, form)
    assert rc == XR_OK, what
    ref = _check_logits(m, weights, form, lg, what)
    want = acs.actions_of(m, ref)
    assert act.tolist() == want.tolist(), what
    assert all(a == 0 for a, n in zip(act.tolist(), case.nlegal) if n <= 0)
    rc2, lg2, act2 = _call(m, weights, form)
    assert rc2 == XR_OK and torch.equal(lg2.view(torch.int32), lg.view(torch.int32)) and torch.equal(act2, act), (what, "two runs differ")
    rc3, none, act3 = _call(m, weights, form, want_logits=False)
    assert rc3 == XR_OK and none is None and torch.equal(act3, act), (what, "logits_dev = NULL")
    rc4, lg4, act4 = _call(m, weights, form, plain=True)
    assert rc4 == XR_OK and torch.equal(lg4.view(torch.int32), lg.view(torch.int32)) and torch.equal(act4, act), (what, "xr_agent_actor")
    sub = list(range(1, case.B, 3))
    if sub:
        rc5, lg5, act5 = _call(m, weights, form, rows=sub)
        assert rc5 == XR_OK and torch.equal(lg5.view(torch.int32), lg[sub].view(torch.int32)) and torch.equal(act5, act[sub]), (what, "sub-batch")


@pytest.mark.parametrize("form", acs.FORMS)
def test_actor_no_envs(form):
    """n_envs = 0: XR_OK through both entry points, nothing written"""
    m = acs.make_case(acs.CASE["none"])
    for kw in (dict(), dict(plain=True), dict(sample=acs.S0)):
        rc, lg, act = _call(m, "plain", form, **kw)                         # (_call holds every element of both outputs to its sentinel)
        assert rc == XR_OK and lg.shape[0] == 0 and act.numel() == 0, (form, kw)


# ---- 2. ties -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", acs.WEIGHT_SETS)
@pytest.mark.parametrize("form", acs.FORMS)
def test_actor_first_maximum_on_ties(form, weights):
    """acs.tie_cases: the maximal logit twice — at ranks (0, 1): one round of the PRE form, its two waves; (1, 2): two rounds; first and last; every vector the
    same.  The action is the id at the LOWER rank (agents.segment_argmax's rule, the header's "first maximum in the channel's order") and the duplicated logits
    are bit-equal.  The duplicated rows of cache_pre are copied bit for bit like those of the cache: this is about the kernel, not about the matrix product
    that fills cache_pre."""
    for kind, m in acs.tie_cases(weights):
        what = f"tie/{kind} {weights} {form}"
        K = m.case.cache_kmax
        pre = None
        if form == "pre":
            pre = _pre(m.vec.to(DEV), weights)
            for e, ids in enumerate(m.ids):
                rows = int(m.region[e]) * K + torch.tensor(ids) - 1
                lo, hi = m.ties[e]
                dst = rows if kind == "all_same" else rows[hi: hi + 1]
                pre[dst.to(DEV)] = pre[int(rows[lo])].clone()
        rc, lg, act = _call(m, weights, form, pre=pre)
        assert rc == XR_OK, what
        _check_logits(m, weights, form, lg, what)
        for e, ids in enumerate(m.ids):
            lo, hi = m.ties[e]
            dup = range(len(ids)) if kind == "all_same" else (lo, hi)
            bits = lg[e].contiguous().view(torch.int32)
            assert all(int(bits[k]) == int(bits[lo]) for k in dup), (what, e, "the duplicated logits differ in bits")
            assert float(lg[e, :len(ids)].max()) == float(lg[e, lo]), (what, e)
            assert int(act[e]) == ids[lo], (what, e, int(act[e]), ids[lo], ids[hi])


# ---- 3. sampling -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", acs.WEIGHT_SETS)
@pytest.mark.parametrize("case,form", RUNS, ids=_rid)
def test_actor_sampling_sweep(case, form, weights):
    """env_ids set (global ids 0, 1, 2^31, 2^40 + 3, ...): the action of EVERY env is the arg-max of acs.sample_scores64 (fp64 logits, the exact fp32 uniforms
    of agents.CounterUniform; the host test holds the top-two distance), it is what CounterUniform and the tensor ops of agents.ppo_actions pick from the kernel's
    own logits, the logits are those of the greedy call, a sub-batch picks what the whole batch picks, and another s0 changes some action."""
    what = f"{case.name} {weights} {form} sampled"
    m = acs.make_case(case)
    rc, lg, act = _call(m, weights, form, sample=acs.S0)
    assert rc == XR_OK, what
    ref = acs.logits64(m, weights)
    want = acs.actions_of(m, acs.sample_scores64(ref, m.env_ids, acs.S0))
    assert act.tolist() == want.tolist(), what
    rc0, lg0, act0 = _call(m, weights, form)
    assert rc0 == XR_OK and torch.equal(lg0.view(torch.int32), lg.view(torch.int32)), (what, "sampling changed the logits")
    # the framework path's tensor ops (agents.ppo_actions, sample_in_kernel=False) on the kernel's logits, on the device
    lgd, kcap = lg.to(DEV), case.kcap
    uni = agents.CounterUniform(0, 0, m.env_ids.to(DEV), _s0=acs.S0)
    ee = torch.arange(case.B, device=DEV).repeat_interleave(kcap)
    u = uni(ee, torch.arange(kcap, device=DEV).repeat(case.B)).reshape(lgd.shape)
    pick = (lgd - torch.log(-torch.log(u))).argmax(dim=1, keepdim=True)
    a = m.head.to(DEV)[:, case.ids_off: case.ids_off + kcap].gather(1, pick)[:, 0].to(torch.int32)
    a = torch.where(m.nlegal.to(DEV) > 0, a, torch.zeros_like(a))
    assert act.tolist() == a.cpu().tolist(), (what, "the tensor ops pick another net")
    sub = list(range(1, case.B, 3))
    if sub:
        rc5, _, act5 = _call(m, weights, form, rows=sub, sample=acs.S0)
        assert rc5 == XR_OK and torch.equal(act5, act[sub]), (what, "sub-batch")
    rc6, _, act6 = _call(m, weights, form, sample=acs.S0_OTHER)
    assert rc6 == XR_OK and act6.tolist() == acs.actions_of(m, acs.sample_scores64(ref, m.env_ids, acs.S0_OTHER)).tolist(), what
    if case.name in acs.S0_MATTERS:                                   # (the host test: the fp64 picks of the two s0 differ there)
        assert not torch.equal(act6, act), (what, "another s0, the same actions")


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------------
def test_actor_refusals_leave_the_outputs_alone():
    """What the launcher refuses, by status, with every element of both guarded outputs still the sentinel (held inside _call): cache_pre with kcap = 257
    (XR_ERR_RANGE; the same arguments without cache_pre run), kcap = 0, a head row one float too short, cache_kmax = 0 and a NULL action_dev (XR_ERR_INVALID)."""
    big = acs.make_case(acs.CASE["over256"])                        # rows of 300 floats: kcap = 257 fits them
    pre = _pre(big.vec.to(DEV), "plain")
    for plain in (False, True):
        rc, lg, act = _call(big, "plain", "pre", pre=pre, kcap=257, plain=plain)
        assert rc == XR_ERR_RANGE and lg.shape[0] == 0 and act.numel() == 0, plain
    m = acs.make_case(acs.CASE["clamp7"])
    c = m.case
    for form in acs.FORMS:
        for over in (dict(kcap=0), dict(head_stride=c.ids_off + c.kcap - 1), dict(cache_kmax=0), dict(action=0), dict(n_envs=-1)):
            if "kcap" in over:                                              # (a logits tensor of no column: nothing to guard, pass NULL)
                rc, _, act = _call(m, "plain", form, want_logits=False, **over)
            else:
                rc, _, act = _call(m, "plain", form, **over)
            assert rc == XR_ERR_INVALID and act.numel() == 0, (form, over, rc)


def test_actor_kcap_257_runs_without_cache_pre():
    """... and one past the PRE form's limit the form without cache_pre answers: kcap = 257 on the rows of 300 ids (nlegal clamped to 257)"""
    m = acs.make_case(acs.CASE["over256"])
    rc, lg, act = _call(m, "plain", "vec", kcap=257)
    assert rc == XR_OK
    ref = acs.logits64(m, "plain")
    for e, r in enumerate(ref):
        n = min(r.numel(), 257)
        assert bool(torch.isfinite(lg[e, :n]).all()) and bool((lg[e, n:] == float("-inf")).all()), e
        assert n == 0 or float((lg[e, :n].double() - r[:n]).abs().max()) <= acs.TOL["plain"], e


# ---- 5. rows that did not parse ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", acs.FORMS)
def test_actor_negative_nlegal_writes_its_own_row_only(form):
    """acs.FLAGGED: rows with nlegal = region = -1 (what xr_batch_expand_state writes for a row that does not parse), each directly behind an env with nlegal ==
    kcap and none first.  The flagged env gets action 0 and a logits row of -inf; every other row is bit-equal to the run without the flagged rows — the
    neighbour's LAST logit included, which a tail fill starting at nl = -1 also writes (-inf) — and the guards are intact.  Greedy and sampled.
    That stray write races with the neighbour's own workgroup writing the same slot, and the neighbour, which has seven nets to evaluate first, usually writes
    last: with an unclamped nl the comparison above passed on an MI355X.  What shows the stray write every time is a slot nobody else writes: the same batch
    with a flagged row FIRST, directly behind the guard rows in front of the logits (inside the allocation) — the last element of the guard row must keep its
    sentinel, which _call asserts."""
    m = acs.make_case(acs.FLAGGED)
    c = m.case
    flagged = [e for e in range(c.B) if c.nlegal[e] < 0]
    others = [e for e in range(c.B) if c.nlegal[e] >= 0]
    for sample in (None, acs.S0):
        first = [flagged[0]] + others + flagged[1:]
        rcf, lgf, actf = _call(m, "plain", form, rows=first, sample=sample)              # (the guards: inside _call)
        assert rcf == XR_OK and int(actf[0]) == 0 and bool((lgf[0] == float("-inf")).all()), form
        rc, lg, act = _call(m, "plain", form, sample=sample)
        rc0, lg0, act0 = _call(m, "plain", form, rows=others, sample=sample)
        assert rc == XR_OK and rc0 == XR_OK
        assert torch.equal(lgf[1: 1 + len(others)].view(torch.int32), lg0.view(torch.int32)) and torch.equal(actf[1: 1 + len(others)], act0), form
        for e in flagged:
            assert float(lg[e - 1, c.kcap - 1]) == float(lg0[others.index(e - 1), c.kcap - 1]), (form, e, "the flagged row overwrote its neighbour's last logit",
                                                                                                float(lg[e - 1, c.kcap - 1]), float(lg0[others.index(e - 1), c.kcap - 1]))
            assert int(act[e]) == 0 and bool((lg[e] == float("-inf")).all()), (form, e)
        assert torch.equal(lg[others].view(torch.int32), lg0.view(torch.int32)) and torch.equal(act[others], act0), form
    _check_logits(m, "plain", form, lg, f"flagged plain {form}")


# ---- 6. more than 256 nets through dqn_actions / ppo_actions -------------------------------------------------------------------------------
def test_more_than_256_nets_through_the_policy_calls():
    """Regions of up to 300 nets through agents.dqn_actions / ppo_actions with the fused kernels: a FusedObstacleTower at the tower sweep's smallest shape, a
    hand-filled complete NetVectorCache of k_max = 300 (acs.CASE["over256"]), head rows of a grid and up to 300 ids.  kcap = 300 is beyond what the kernel takes
    together with cache_pre: FusedActorHead launches without it.  The calls do not raise, return the fp64 actions computed from tower(head) as the state — greedy,
    sampled in the kernel and sampled by the tensor ops —, build no cache._pre, and the tower is still `supported`."""
    m = acs.make_case(acs.CASE["over256"])
    c = m.case
    D, H, W = acs.PY_SHAPE
    N = D * H * W
    model = agents.ActorCritic(64)
    model.representation_network = copy.deepcopy(ts.make_rep("plain"))
    model.actor = copy.deepcopy(acs.make_actor("plain"))
    model = model.to(DEV).eval()
    tower = agents.FusedObstacleTower(model.representation_network, acs.PY_SHAPE, DEV)
    actor = agents.FusedActorHead(model.actor, DEV)
    assert tower.supported and c.kcap > acs.IDS_MAX
    cache = agents.NetVectorCache(c.n_regions, c.cache_kmax, DEV)
    cache.vec.copy_(m.vec)
    cache.valid.copy_(torch.isfinite(m.vec).all(dim=1))
    cache.complete, cache.computed = True, int(cache.valid.sum())
    head = acs.py_head(m).to(DEV)
    nlegal, region = m.nlegal.to(DEV), m.region.to(DEV)
    kw = dict(cache=cache, region=region, ob_tower=tower, actor_head=actor)
    dims = (W, H, D)
    assert agents._fused_ready(kw, dims, head)
    state = tower(head)
    ref = acs.logits64(m, "plain", state=state.cpu())
    gap, sgap = acs.top_gap(ref), acs.top_gap(acs.sample_scores64(ref, m.env_ids, acs.S0))
    assert gap >= acs.GAP * acs.TOL["plain"] and sgap >= acs.SCORE_GAP, (gap, sgap)
    a_dqn = agents.dqn_actions(model, head, nlegal, dims, **kw)
    assert a_dqn.cpu().tolist() == acs.actions_of(m, ref).tolist()
    uni = agents.CounterUniform(0, 0, m.env_ids.to(DEV), _s0=acs.S0)
    want = acs.actions_of(m, acs.sample_scores64(ref, m.env_ids, acs.S0)).tolist()
    a_k, v_k = agents.ppo_actions(model, head, nlegal, dims, uniform=uni, **kw)
    a_t, v_t = agents.ppo_actions(model, head, nlegal, dims, uniform=uni, sample_in_kernel=False, **kw)
    assert a_k.cpu().tolist() == want and a_t.cpu().tolist() == want
    assert torch.equal(v_k, v_t) and v_k.shape == (c.B,)
    assert tower.supported and getattr(cache, "_pre", None) is None and actor.PRE_KCAP_MAX == acs.IDS_MAX
    # the kernel's logits, through the head's own call, against the same reference
    _, lg = actor(state, head, N, nlegal, region, cache, c.kcap, want_logits=True)
    err = max(float((lg[e, :r.numel()].double().cpu() - r).abs().max()) for e, r in enumerate(ref) if r.numel())
    print(f"ACTOR_ERR python/over256 plain vec {err:.2e}")
    assert err <= acs.TOL["plain"], err
