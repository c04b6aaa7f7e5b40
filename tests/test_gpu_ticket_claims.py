"""How the step kernel hands out slab tickets, against the oracle and against xr_batch_observation, where the hand-out can go wrong.

A queue-form launch whose tickets are slabs (fp32, aligned planes, S > 1: the largest region has more than 3 tiles of 1024 nodes)
issues a workgroup's next claim after the current ticket's stores; every other launch (S = 1) claims before them.  A workgroup's first
ticket is static and the counter hands out the rest, so what a launch writes depends on its grid: min(obs_writer_blocks or the chip's
capacity, 4 * n_envs).  Here: batches of 1, 2, 3 and 9 envs (grids of 4, 8, 12 and 36, more workgroups than tickets at an episode's
end), writer-block counts of 1, 3, 13 and 27, N = 8640 (9 tiles, the last partial), regions of 1028 nodes (2 tiles, the second nearly
empty) and of 4 nodes alone (S = 1) and beside N = 8640 (S = 3: their later slabs are empty tickets), a launch with routes and no unit,
six consecutive steps into one buffer (the counters of the next call are zeroed by this call's plan, two banks: a bank that is not
zeroed drops tickets on the third call), the in-place form, invalid actions, and group steps between batch-wide steps with one group
per slot.  The shapes were chosen for per-XCD ticket heads with stealing (LAB_NOTES.md, section 21: measured slower, not in the
tree); they pin the single counter just as well.

Every check: sentinel-filled buffer (full write) or the previous observation (in place), rows against oracle.build_observation of the
fetched state, and the whole buffer byte for byte against xr_batch_observation of the same state (a sequence of in-place steps: after
its last step, since the stand-alone observation takes over the in-place bookkeeping)."""
import gc

import pytest
import torch

from tests.helpers import SENTINEL_F32, assert_rows_match_oracle
from xroute_env_amd import _lib
from xroute_env_amd.batch import RegionBatch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x7EAD
SENT = SENTINEL_F32

SHAPES = {
    "workload": [(24, 40, 9)],                               # N 8640: 9 tiles, the last one partial; S = 3
    "n1028": [(257, 2, 2)],                                  # 2 tiles, the second holds one float4; S = 1: the single head
    "n4": [(2, 2, 1)],                                       # one float4 per plane; S = 1
    "mixed_1028": [(24, 40, 9), (257, 2, 2)],                # S = 3 from n_max: the small region's slabs 1..2 are empty tickets
    "mixed_4": [(24, 40, 9), (2, 2, 1)],
}
_regions = {}


@pytest.fixture(autouse=True)
def _release_cached_memory():
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _set_regions(name, reps=2):
    """`reps` regions per shape with at least 2 nets each (N = 4: as many as fit); deterministic, generated once."""
    if name not in _regions:
        from xroute_env_amd.regions import generate_region
        out, seed = [], 9400
        for d in SHAPES[name]:
            got, need = 0, (1 if d[0] * d[1] * d[2] < 16 else 2)
            while got < reps:
                r = generate_region(seed, dims=d, k_range=(1, 9), net_span=4)
                seed += 1
                if r.n_nets >= need:
                    assert r.n_nodes % 4 == 0
                    out.append(r)
                    got += 1
        _regions[name] = out
    return _regions[name]


def _batch(name, n_envs, **kw):
    return RegionBatch(_set_regions(name), n_envs=n_envs, device=DEV, auto_reset=True, max_route_count=1, **kw)


def _buffer(batch):
    buf = torch.full((batch.n_envs, batch.obs_env_stride), SENT, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    return buf


def _check(batch, buf, full_write, what, compare_obs=True):
    """Rows against the oracle; then the buffer against xr_batch_observation of the same state, byte for byte (in place: wherever the
    stand-alone observation wrote; older planes may remain behind a row that got shorter).  The stand-alone observation makes ITS
    buffer the one that holds the batch's observation, so a sequence of in-place steps compares with it after its last step only."""
    n = batch.n_envs
    regs = assert_rows_match_oracle(batch, buf, 0, n, SENT, full_write, what)
    if not compare_obs:
        return regs
    ref = torch.full_like(buf, SENT)
    batch.observation(ref)
    a, r = buf.view(torch.int32), ref.view(torch.int32)
    if full_write:
        assert torch.equal(a, r), (what, "step observation != xr_batch_observation")
    else:
        m = ref != SENT
        assert torch.equal(a[m], r[m]), (what, "step observation != xr_batch_observation")
    return regs


def _steps(batch, buf, inplace, steps, what, reject_at=(1,)):
    """`steps` consecutive batch-wide steps into the SAME buffer; step `reject_at` carries invalid actions (0 and an id past every net)."""
    n = batch.n_envs
    act = torch.empty(n, dtype=torch.int32, device=DEV)
    if inplace:
        batch.observation(buf)
    rejected = 0
    for t in range(steps):
        batch.random_actions(SEED + t, act)
        if t in reject_at:
            act[::2] = 9999
            act[1::4] = 0
        if not inplace:
            buf.fill_(SENT)
        batch.step(act, buf, inplace=inplace)
        info = batch.observe_info()
        assert info["form"] == 3 and info["inplace"] == inplace, (what, t, info)
        if t in reject_at:
            rejected += int((batch.fetch("status") & _lib.XR_ENV_BAD_ACTION).ne(0).sum())
        _check(batch, buf, not inplace, (what, t), compare_obs=not inplace or t == steps - 1)
    assert rejected > 0 or not reject_at


@pytest.mark.parametrize("inplace", [False, True], ids=["full", "inplace"])
@pytest.mark.parametrize("n_envs", [1, 2, 3, 9])
@pytest.mark.parametrize("name", ["workload", "mixed_1028"])
def test_small_batches(name, n_envs, inplace):
    """Grids of 4, 8, 12 and 36 workgroups."""
    batch = _batch(name, n_envs)
    batch.reset(rotate=True)
    _steps(batch, _buffer(batch), inplace, 6, (name, n_envs, inplace))


@pytest.mark.parametrize("inplace", [False, True], ids=["full", "inplace"])
@pytest.mark.parametrize("name", ["n1028", "n4", "mixed_4"])
def test_small_regions(name, inplace):
    batch = _batch(name, 9)
    batch.reset(rotate=True)
    _steps(batch, _buffer(batch), inplace, 6, (name, inplace))


@pytest.mark.parametrize("blocks", [1, 3, 13, 27])
@pytest.mark.parametrize("name", ["workload", "mixed_1028"])
def test_writer_blocks_not_a_multiple_of_8(name, blocks):
    """17 envs (up to 68 workgroups) capped at 1, 3, 13 and 27 workgroups; one workgroup takes every route and every ticket itself."""
    batch = _batch(name, 17, obs_writer_blocks=blocks)
    batch.reset(rotate=True)
    _steps(batch, _buffer(batch), False, 6, (name, blocks))


@pytest.mark.parametrize("n_envs", [3, 17])
def test_zero_units_on_the_last_net(n_envs):
    """Every env plays the same region to its last net (no auto-reset): that step's launch has routes and no unit, and the calls
    after it find their counters zeroed like every other call."""
    region = _set_regions("workload")[0]
    batch = RegionBatch([region], n_envs=n_envs, device=DEV, auto_reset=False, max_route_count=1)
    batch.reset()
    buf = _buffer(batch)
    act = torch.empty(n_envs, dtype=torch.int32, device=DEV)
    left = int(batch.fetch("nlegal").sum())
    assert left >= 2 * n_envs
    for t in range(region.n_nets):
        batch.random_actions(SEED + 50 + t, act)
        buf.fill_(SENT)
        batch.step(act, buf)
        assert batch.observe_info()["form"] == 3
        left = int(batch.fetch("nlegal").sum())
        assert left > 0 or int(batch.fetch("units").item()) == 0       # (queue[2] counts units, whatever hands the tickets out)
        _check(batch, buf, True, ("last net", n_envs, t))
        if left == 0:
            break
    assert left == 0
    batch.reset()
    for t in range(3):
        batch.random_actions(SEED + 70 + t, act)
        buf.fill_(SENT)
        batch.step(act, buf)
        _check(batch, buf, True, ("after the zero-unit launch", n_envs, t))


@pytest.mark.parametrize("inplace", [False, True], ids=["full", "inplace"])
def test_group_steps_between_batch_wide_steps(inplace):
    """One group per slot (17 groups, each with counters of its own), every group on one of two streams; rounds of group steps
    alternate with batch-wide steps into the same buffer."""
    name = "mixed_1028"
    batch = _batch(name, 17)
    n = batch.n_envs
    batch.set_groups(n)
    buf = _buffer(batch)
    batch.reset(rotate=True)
    if inplace:
        batch.observation(buf)
    cur = torch.cuda.current_stream()
    streams = [torch.cuda.Stream() for _ in range(2)]
    act = torch.empty(n, dtype=torch.int32, device=DEV)
    gacts = []
    for g in range(n):
        s = streams[g & 1]
        s.wait_stream(cur)
        with torch.cuda.stream(s):
            gacts.append(torch.empty(1, dtype=torch.int32, device=DEV))
    kinds = "bgbgbbgg"                                        # batch-wide and group rounds; each kind twice in a row once
    for rnd, kind in enumerate(kinds):
        if not inplace:
            buf.fill_(SENT)
        if kind == "b":
            batch.random_actions(SEED + 200 + rnd, act)
            if rnd == 2:
                act[::2] = 9999
            batch.step(act, buf, inplace=inplace)
        else:
            for s in streams:
                s.wait_stream(cur)
            for g in range(n):
                s = streams[g & 1]
                with torch.cuda.stream(s):
                    batch.random_actions_group(g, SEED + 300 + rnd, out=gacts[g], stream=s)
                    batch.step_group(g, gacts[g], buf[g:g + 1], inplace=inplace, stream=s)
            for s in streams:
                cur.wait_stream(s)
        torch.cuda.synchronize()
        info = batch.observe_info()
        # (a buffer holds the previous observation for a call of the same kind only: a batch-wide step invalidates the groups' and back)
        want_inplace = inplace and (rnd == 0 or kinds[rnd - 1] == kind)
        assert info["form"] == 3 and info["inplace"] == want_inplace, (rnd, info)
        _check(batch, buf, not inplace, (name, "groups", inplace, rnd), compare_obs=not inplace or rnd == len(kinds) - 1)
