"""The step kernel's slab tickets against the oracle, at the shapes where the ticket decode can go wrong.

The queue form's unit counter hands out tickets: ticket t = slab t % S of unit t / S, a slab = XR_TICKET_TILES (3) tiles of 1024 nodes,
S = ceil(ceil(n_max / 1024) / 3) from the batch's largest region.  The shape table of tests/test_gpu_obs_writers.py has N = 640 and
8640 only among aligned shapes; here: units of exactly one and two full tiles, a one-float4 tail tile, the 9-tile boundary, 12 tiles
(S = 4), the workload's own shape (S = 3, last tile partial), and batches that mix region sizes, where small regions' later slabs are
empty and u / p are decoded across regions of different N.  Batches whose largest region has at most 3 tiles run with S = 1.
Every case: sentinel-filled buffer, rows against oracle.build_observation of the fetched state (never a twin of the same kernel),
nothing written behind (2+7K)N in a full write, auto-reset with rotation, rejected actions, observe_info()["form"] == 3."""
import gc

import pytest
import torch

from tests.helpers import SENTINEL_F32, assert_rows_match_oracle
from xroute_env_amd import _lib
from xroute_env_amd.batch import RegionBatch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x51AB
SENT = SENTINEL_F32

# name -> dims of the regions of one batch (N = X * Y * Z, all N % 4 == 0)
SLAB_SHAPES = {
    "one_tile_full": [(16, 16, 4)],                          # N 1024: a unit is exactly one tile
    "two_tiles_full": [(32, 16, 4)],                         # N 2048: the last tile is full, an off-by-one writes past the unit
    "tail_one_group": [(257, 2, 2)],                         # N 1028: the second tile holds one float4
    "nine_tiles_full": [(48, 48, 4)],                        # N 9216: the 9-tile boundary, S = 3, no partial tile
    "twelve_tiles": [(32, 40, 9)],                           # N 11520: S = 4 (was a second pass of the whole-unit writer)
    "workload": [(24, 40, 9)],                               # N 8640: 9 tiles, the last one partial
    "mixed": [(32, 40, 9), (16, 10, 4), (257, 2, 2)],        # S = 4 from n_max; the small regions' slabs 1..3 are empty
    "mixed_full_tiles": [(24, 40, 9), (16, 16, 4), (32, 16, 4)],      # S = 3; units of exactly 1 and 2 tiles beside empty slabs
}
BOUNDS = [0, 1, 7, 13, 17]
_regions = {}


@pytest.fixture(autouse=True)
def _release_cached_memory():
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _set_regions(name):
    """Three regions per shape (slots rotate to another K), each with at least 2 nets; deterministic, generated once."""
    if name not in _regions:
        from xroute_env_amd.regions import generate_region
        out, seed = [], 9100
        for d in SLAB_SHAPES[name]:
            got = 0
            while got < 3:
                r = generate_region(seed, dims=d, k_range=(1, 9), net_span=4)
                seed += 1
                if r.n_nets >= 2:
                    assert r.n_nodes % 4 == 0
                    out.append(r)
                    got += 1
        _regions[name] = out
    return _regions[name]


def _batch(name, n_envs=17):
    return RegionBatch(_set_regions(name), n_envs=n_envs, device=DEV, auto_reset=True, max_route_count=1)


def _buffer(batch, extra=0):
    buf = torch.full((batch.n_envs, batch.obs_env_stride + extra), SENT, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    return buf


def _reject_some(act):
    act[::3] = 0
    act[1::3] = 9999


def _steps(batch, buf, inplace, steps, what):
    """`steps` whole-batch steps into `buf`, every row against the oracle after each; returns the region tuples seen."""
    n = batch.n_envs
    act = torch.empty(n, dtype=torch.int32, device=DEV)
    if inplace:
        batch.observation(buf)
        assert_rows_match_oracle(batch, buf, 0, n, SENT, True, (what, "primed"))
    seen, rejected = set(), 0
    for t in range(steps):
        batch.random_actions(SEED + t, act)
        if t in (1, 2):
            _reject_some(act)
        if not inplace:
            buf.fill_(SENT)
        batch.step(act, buf, inplace=inplace)
        info = batch.observe_info()
        assert info["form"] == 3 and info["inplace"] == inplace, (what, t, info)
        if t in (1, 2):
            rejected += int((batch.fetch("status") & _lib.XR_ENV_BAD_ACTION).ne(0).sum())
        seen.add(tuple(assert_rows_match_oracle(batch, buf, 0, n, SENT, not inplace, (what, t))))
    assert rejected > 0
    return seen


FORMS = {"full": (False, 0), "stride_plus4": (False, 4), "inplace": (True, 0)}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", SLAB_SHAPES)
def test_step_matches_oracle(name, form):
    inplace, extra = FORMS[form]
    batch = _batch(name)
    batch.reset(rotate=True)
    seen = _steps(batch, _buffer(batch, extra), inplace, 12, (name, form))  # (9 nets at most + 2 steps of rejections: every first episode ends)
    assert len(seen) > 1                                     # slots finished, re-initialised and rotated on the way


@pytest.mark.parametrize("inplace", [False, True], ids=["full", "inplace"])
@pytest.mark.parametrize("name", SLAB_SHAPES)
def test_group_steps_match_oracle(name, inplace):
    """One env-group partition, every group on its own stream (a group's launch has its own counters and its own slice of the units)."""
    batch = _batch(name)
    n, G = batch.n_envs, len(BOUNDS) - 1
    batch.set_groups(BOUNDS)
    buf = _buffer(batch)
    batch.reset(rotate=True)
    if inplace:
        batch.observation(buf)
        assert_rows_match_oracle(batch, buf, 0, n, SENT, True, (name, "groups", "primed"))
    cur = torch.cuda.current_stream()
    streams = [torch.cuda.Stream() for _ in range(G)]
    acts = []
    for g, s in enumerate(streams):
        s.wait_stream(cur)
        with torch.cuda.stream(s):
            acts.append(torch.empty(BOUNDS[g + 1] - BOUNDS[g], dtype=torch.int32, device=DEV))
    seen, rejected = set(), 0
    for rnd in range(12):
        for g in range(G):
            lo, hi = BOUNDS[g], BOUNDS[g + 1]
            with torch.cuda.stream(streams[g]):
                batch.random_actions_group(g, SEED + 100 + rnd, out=acts[g], stream=streams[g])
                if rnd in (1, 2):
                    _reject_some(acts[g])
                if not inplace:
                    buf[lo:hi].fill_(SENT)
                batch.step_group(g, acts[g], buf[lo:hi], inplace=inplace, stream=streams[g])
            info = batch.observe_info()
            assert info["form"] == 3 and info["inplace"] == inplace, (name, g, rnd, info)
        for s in streams:
            cur.wait_stream(s)
        torch.cuda.synchronize()
        if rnd in (1, 2):
            rejected += int((batch.fetch("status") & _lib.XR_ENV_BAD_ACTION).ne(0).sum())
        seen.add(tuple(assert_rows_match_oracle(batch, buf, 0, n, SENT, not inplace, (name, "groups", rnd))))
    assert rejected > 0
    assert len(seen) > 1


@pytest.mark.parametrize("n_envs", [1, 3])
@pytest.mark.parametrize("name", ["workload", "twelve_tiles", "mixed"])
def test_fewer_tickets_than_workgroups(name, n_envs):
    """1 and 3 slots: the launch has more workgroups than tickets at the end of an episode, and the static first tickets run past the end."""
    batch = _batch(name, n_envs=n_envs)
    batch.reset(rotate=True)
    _steps_small(batch, _buffer(batch), (name, n_envs))


def _steps_small(batch, buf, what):
    n = batch.n_envs
    act = torch.empty(n, dtype=torch.int32, device=DEV)
    for t in range(12):                                      # (through the end of every slot's first episode: at most 9 nets)
        batch.random_actions(SEED + 300 + t, act)
        if t == 2:
            act[0] = 9999
        buf.fill_(SENT)
        batch.step(act, buf)
        assert batch.observe_info()["form"] == 3, (what, t)
        assert_rows_match_oracle(batch, buf, 0, n, SENT, True, (what, t))


@pytest.mark.parametrize("name", ["workload", "mixed"])
def test_step_with_zero_units(name):
    """Every action rejected, in place: no slot's net set changes, the plan lists no unit, and the launch has no ticket to hand out."""
    batch = _batch(name)
    n = batch.n_envs
    batch.reset(rotate=True)
    buf = _buffer(batch)
    act = torch.empty(n, dtype=torch.int32, device=DEV)
    batch.observation(buf)
    for t, bad in enumerate((9999, 0)):
        act.fill_(bad)
        batch.step(act, buf, inplace=True)
        info = batch.observe_info()
        assert info["form"] == 3 and info["inplace"] == True, info      # noqa: E712
        assert int((batch.fetch("status") & _lib.XR_ENV_BAD_ACTION).ne(0).sum()) == n
        assert int(batch.fetch("units").item()) == 0             # (queue[2] keeps counting units, not tickets)
        assert_rows_match_oracle(batch, buf, 0, n, SENT, True, (name, "zero units", t))
    batch.random_actions(SEED + 400, act)                    # and the next real step still writes what changed
    batch.step(act, buf, inplace=True)
    assert_rows_match_oracle(batch, buf, 0, n, SENT, False, (name, "after zero units"))
