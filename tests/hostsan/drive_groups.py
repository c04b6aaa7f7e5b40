"""Driver of tests/test_env_groups_host.py: the env-group entry points (xr_batch_set_groups / _step_group / _random_actions_group /
_fetch_group) of the product's host C++ under ASan + UBSan, against the host-memory HIP stand-in of this directory (argv: repo root,
library).  Valid partitions run every staging path; a few thousand seeded hostile partitions, groups, strides and sizes must be refused
with a status, never read or write outside a buffer, and leave the batch usable.  Ends without a leaked device buffer."""
import ctypes as C
import sys

import numpy as np

sys.path.insert(0, sys.argv[1])
from xroute_env_amd import _lib as X                      # ctypes structures only: the module does not load the real library
from xroute_env_amd.regions import generate_region

L = C.CDLL(sys.argv[2])
vp = C.c_void_p
L.xr_last_error.restype = C.c_char_p
L.xr_config_default.argtypes = [C.POINTER(X.XrConfig)]; L.xr_config_default.restype = None
L.xr_batch_create.argtypes = [C.POINTER(X.XrConfig), C.POINTER(vp)]
L.xr_batch_destroy.argtypes = [vp]
L.xr_batch_load_regions.argtypes = [vp, C.POINTER(X.XrRegionDesc), C.c_int32, vp]
L.xr_batch_sizes.argtypes = [vp] + [C.POINTER(C.c_int32)] * 6 + [C.POINTER(C.c_int64)]
L.xr_batch_step_observe_inplace.argtypes = [vp, vp, vp, C.c_int64, vp]
L.xr_batch_observation.argtypes = [vp, vp, C.c_int64, C.c_int32, C.c_int32, vp]
L.xr_batch_observe_timing.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_float)]
L.xr_batch_reset.argtypes = [vp, vp, C.c_int32, vp]
L.xr_batch_set_groups.argtypes = [vp, vp, C.c_int32]
L.xr_batch_step_group.argtypes = [vp, C.c_int32, vp, vp, C.c_int64, C.c_int32, vp]
L.xr_batch_random_actions_group.argtypes = [vp, C.c_int32, vp, C.c_uint64, vp]
L.xr_batch_fetch_group.argtypes = [vp, C.c_int32, C.c_int32, vp, C.c_size_t, vp]
live = C.c_int64.in_dll(L, "xr_stub_alloc_live")
launches = C.c_int64.in_dll(L, "xr_stub_launches")
rng = np.random.default_rng(2024)
counts = {}


def note(rc):
    counts[rc] = counts.get(rc, 0) + 1
    return rc


def create(**kw):
    c = X.XrConfig(); L.xr_config_default(C.byref(c))
    for k, v in kw.items():
        setattr(c, k, v)
    h = vp()
    assert L.xr_batch_create(C.byref(c), C.byref(h)) == 0, kw
    return h


keep = []


def load(h, regs):
    arr = (X.XrRegionDesc * len(regs))()
    for d, r in zip(arr, regs):
        xs, ys = np.ascontiguousarray(r.xs, np.int32), np.ascontiguousarray(r.ys, np.int32)
        ld, nodes = np.ascontiguousarray(r.layer_dir, np.uint8), np.ascontiguousarray(r.nodes, np.uint32)
        keep.extend([xs, ys, ld, nodes])
        d.dim_x, d.dim_y, d.dim_z = r.dims
        d.xs_host, d.ys_host, d.layer_dir_host, d.nodes_host = xs.ctypes.data, ys.ctypes.data, ld.ctypes.data, nodes.ctypes.data
        d.n_nets = r.n_nets
        for j in range(3):
            d.metrics0[j] = int(r.metrics0[j])
    return L.xr_batch_load_regions(h, arr, len(regs), None)


def set_groups(h, bounds):
    a = np.ascontiguousarray(bounds, np.int32)
    return L.xr_batch_set_groups(h, a.ctypes.data if a.size else None, max(a.size - 1, 0))


# ---- null arguments, and every entry point before load_regions
assert L.xr_batch_set_groups(None, None, 1) == X.XR_ERR_INVALID
assert L.xr_batch_step_group(None, 0, None, None, 0, 0, None) == X.XR_ERR_INVALID
assert L.xr_batch_random_actions_group(None, 0, None, 1, None) == X.XR_ERR_INVALID
assert L.xr_batch_fetch_group(None, 0, X.XR_FETCH_HASH, None, 0, None) == X.XR_ERR_INVALID
h = create(n_envs=6)
buf = np.zeros(1 << 12, np.uint8); p = buf.ctypes.data
assert L.xr_batch_step_group(h, 0, p, None, 0, 0, None) == X.XR_ERR_STATE
assert L.xr_batch_random_actions_group(h, 0, p, 1, None) == X.XR_ERR_STATE
assert L.xr_batch_fetch_group(h, 0, X.XR_FETCH_HASH, p, 48, None) == X.XR_ERR_STATE
assert set_groups(h, [0, 2, 6]) == 0                      # a partition may be declared before the regions: it survives the load
L.xr_batch_destroy(h)
assert live.value == 0, ("leaked device bytes", live.value)

# per-env row bytes of every selector xr_batch_fetch_group accepts
def row_bytes(lw, pc, nm):
    return {X.XR_FETCH_RECORD: 48, X.XR_FETCH_REWARD: 8, X.XR_FETCH_DONE: 1, X.XR_FETCH_NLEGAL: 4, X.XR_FETCH_STATUS: 4, X.XR_FETCH_LEGAL: 8 * lw,
            X.XR_FETCH_DELTA: 12, X.XR_FETCH_CUM: 12, X.XR_FETCH_PATH_LEN: 4, X.XR_FETCH_PATH: 4 * pc, X.XR_FETCH_OWNER: 2 * nm, X.XR_FETCH_HASH: 8,
            X.XR_FETCH_REGION: 4, X.XR_FETCH_SWEEPS: 4, X.XR_FETCH_REPLAY: 4, X.XR_FETCH_ENV_STEPS: 8}


cfgs = [dict(n_envs=1), dict(n_envs=7), dict(n_envs=70, router=1), dict(n_envs=9, stream_per_region=1), dict(n_envs=5, obs_mode=2),
        dict(n_envs=12, obs_helper_blocks=4), dict(n_envs=130, launch_order=2), dict(n_envs=3, force_scratch_field=1),
        dict(n_envs=4, guide_cost=500, maze_end_iter=3)]
shapes = [((7, 5, 3), (2, 6)), ((24, 40, 9), (4, 12)), ((6, 6, 12), (1, 5))]
n_ok = 0
for ci, kw in enumerate(cfgs):
    B = kw["n_envs"]
    h = create(**kw)
    d, k = shapes[ci % len(shapes)]
    regs = [generate_region(7000 + 10 * ci + j, dims=d, k_range=k, net_span=4) for j in range(1 + ci % 2)]
    assert load(h, regs) == 0, (kw, L.xr_last_error())
    ne, nr, nm, km, lw, pc = (C.c_int32() for _ in range(6)); st = C.c_int64()
    assert L.xr_batch_sizes(h, C.byref(ne), C.byref(nr), C.byref(nm), C.byref(km), C.byref(lw), C.byref(pc), C.byref(st)) == 0
    stride, need = st.value, (2 + 7 * km.value) * max(r.n_nodes for r in regs)
    rows = row_bytes(lw.value, pc.value, nm.value)
    for trial in range(400):
        # hostile partitions: wrong ends, empty / descending groups, too many groups, n_groups that does not match the array
        G = int(rng.integers(1, min(B, X.XR_MAX_GROUPS) + 1))
        cuts = np.sort(rng.choice(np.arange(1, B), G - 1, replace=False)) if G > 1 else np.zeros(0, np.int64)
        good = np.concatenate([[0], cuts, [B]]).astype(np.int32)
        kind = trial % 5
        if kind == 1:
            bad = good.copy(); bad[int(rng.integers(0, bad.size))] += int(rng.choice([-1, 1])) * int(rng.integers(1, 3))
            rc = note(set_groups(h, bad))
            ok = bad[0] == 0 and bad[-1] == B and np.all(np.diff(bad) > 0)
            assert (rc == 0) == bool(ok), (bad, rc)
            assert rc in (0, X.XR_ERR_INVALID), rc
            if rc != 0:
                assert set_groups(h, good) == 0
            else:
                good = bad                                # (the change kept the bounds valid: that is the partition now)
        elif kind == 2:
            assert note(set_groups(h, np.arange(X.XR_MAX_GROUPS + 2, dtype=np.int32))) in (X.XR_ERR_RANGE, X.XR_ERR_INVALID)
            assert note(L.xr_batch_set_groups(h, good.ctypes.data, 0)) == X.XR_ERR_RANGE
            assert note(L.xr_batch_set_groups(h, good.ctypes.data, -3)) == X.XR_ERR_RANGE
            assert set_groups(h, good) == 0
        else:
            assert set_groups(h, good) == 0, (good, L.xr_last_error())
        n_ok += 1
        Gs = good.size - 1
        # group index out of range
        g_bad = int(rng.choice([-1, Gs, Gs + int(rng.integers(0, 100)), -(1 << 30)]))
        act = np.ones(B, np.int32)
        assert note(L.xr_batch_step_group(h, g_bad, act.ctypes.data, None, 0, 0, None)) == X.XR_ERR_RANGE
        assert note(L.xr_batch_random_actions_group(h, g_bad, act.ctypes.data, 3, None)) == X.XR_ERR_RANGE
        assert note(L.xr_batch_fetch_group(h, g_bad, X.XR_FETCH_HASH, p, 8, None)) == X.XR_ERR_RANGE
        g = int(rng.integers(0, Gs))
        lo, hi = int(good[g]), int(good[g + 1])
        ga = np.ones(hi - lo, np.int32)
        out = np.zeros(64, np.float32)
        # steps: route only, observation with hostile strides and flags
        assert L.xr_batch_step_group(h, g, ga.ctypes.data, None, 0, 0, None) == 0
        assert note(L.xr_batch_step_group(h, g, None, None, 0, 0, None)) == X.XR_ERR_INVALID
        assert note(L.xr_batch_step_group(h, g, ga.ctypes.data, out.ctypes.data, int(rng.integers(-5, need)), 0, None)) == X.XR_ERR_RANGE
        assert note(L.xr_batch_step_group(h, g, ga.ctypes.data, out.ctypes.data, stride, int(rng.integers(2, 1 << 20)), None)) == X.XR_ERR_INVALID
        for flags in (0, X.XR_GROUP_INPLACE, X.XR_GROUP_INPLACE):
            assert L.xr_batch_step_group(h, g, ga.ctypes.data, out.ctypes.data, stride, flags, None) == 0, L.xr_last_error()
        assert L.xr_batch_random_actions_group(h, g, ga.ctypes.data, int(rng.integers(0, 1 << 62)), None) == 0
        # whole-batch calls in between (the in-place bookkeeping of both kinds)
        if trial % 7 == 0:
            assert L.xr_batch_observation(h, out.ctypes.data, stride, 0, B, None) == 0
            assert L.xr_batch_step_observe_inplace(h, act.ctypes.data, out.ctypes.data, stride, None) == 0
            i32, f32 = C.c_int32(), C.c_float()
            assert L.xr_batch_observe_timing(h, C.byref(i32), C.byref(f32)) == 0
            assert L.xr_batch_reset(h, None, 1, None) == 0
        # fetches: exact-size buffers (a red zone right behind them); one byte off either way, batch-wide and unknown selectors refused
        for what, rb in rows.items():
            nb = (hi - lo) * rb
            exact = np.zeros(nb, np.uint8)
            assert L.xr_batch_fetch_group(h, g, what, exact.ctypes.data, nb, None) == 0, (what, L.xr_last_error())
            assert note(L.xr_batch_fetch_group(h, g, what, exact.ctypes.data, nb - 1, None)) == X.XR_ERR_RANGE
            assert note(L.xr_batch_fetch_group(h, g, what, exact.ctypes.data, nb + int(rng.integers(1, 9)), None)) == X.XR_ERR_RANGE
        for what in (X.XR_FETCH_STEPS, X.XR_FETCH_UNITS, X.XR_FETCH_ROUTE_ORDER, -1, 21, int(rng.integers(22, 1 << 30))):
            assert note(L.xr_batch_fetch_group(h, g, what, p, 8, None)) == X.XR_ERR_INVALID
    # a reload keeps the partition; one group restores the default
    assert load(h, regs) == 0
    assert L.xr_batch_step_group(h, Gs - 1, np.ones(B, np.int32).ctypes.data, None, 0, 0, None) == 0
    assert set_groups(h, [0, B]) == 0
    assert L.xr_batch_step_group(h, 1, act.ctypes.data, None, 0, 0, None) == X.XR_ERR_RANGE
    assert L.xr_batch_step_group(h, 0, act.ctypes.data, None, 0, 0, None) == 0
    L.xr_batch_destroy(h)
    assert live.value == 0, ("leaked device bytes", live.value, kw)
print("HOSTSAN_GROUPS_OK", n_ok, launches.value, sorted(counts.items()))
