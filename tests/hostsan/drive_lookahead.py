"""Driver of tests/test_lookahead_host.py: the validators of xr_batch_lookahead in the product's host C++ under ASan + UBSan, against the
host-memory HIP stand-in of this directory (argv: repo root, library).  That build has no lookahead kernels (the launchers are weak
symbols the stand-in does not define): every refusal must come with its documented code BEFORE the host notices, and a call with valid
arguments must answer XR_ERR_STATE without having allocated or launched anything.  Ends without a leaked device buffer."""
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
L.xr_batch_set_groups.argtypes = [vp, vp, C.c_int32]
L.xr_batch_step.argtypes = [vp, vp, vp]
L.xr_batch_lookahead.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp, vp]
live = C.c_int64.in_dll(L, "xr_stub_alloc_live")
launches = C.c_int64.in_dll(L, "xr_stub_launches")
rng = np.random.default_rng(515)
keep = []


def create(**kw):
    c = X.XrConfig(); L.xr_config_default(C.byref(c))
    for k, v in kw.items():
        setattr(c, k, v)
    h = vp()
    assert L.xr_batch_create(C.byref(c), C.byref(h)) == 0, kw
    return h


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


def err():
    return L.xr_last_error().decode()


buf = np.zeros(1 << 16, np.uint8); p = buf.ctypes.data
# null batch / null out, and misuse before the regions are loaded
assert L.xr_batch_lookahead(None, -1, None, p, 4, None, None) == X.XR_ERR_INVALID and "null" in err()
h = create(n_envs=6)
assert L.xr_batch_lookahead(h, -1, None, None, 4, None, None) == X.XR_ERR_INVALID and "null" in err()
assert L.xr_batch_lookahead(h, -1, None, p, 4, None, None) == X.XR_ERR_STATE and "load regions" in err()
assert L.xr_batch_lookahead(h, 0, None, p, 1 << 30, p, None) == X.XR_ERR_STATE
L.xr_batch_destroy(h)
assert live.value == 0

n_checked = 0
cfgs = [dict(n_envs=1), dict(n_envs=7), dict(n_envs=40, router=1), dict(n_envs=9, router=3), dict(n_envs=4, guide_cost=500, maze_end_iter=3),
        dict(n_envs=3, force_scratch_field=1), dict(n_envs=9, stream_per_region=1)]
shapes = [((7, 5, 3), (2, 6)), ((24, 40, 9), (4, 12)), ((6, 6, 12), (1, 5))]
for ci, kw in enumerate(cfgs):
    B = kw["n_envs"]
    h = create(**kw)
    d, k = shapes[ci % len(shapes)]
    regs = [generate_region(7300 + 10 * ci + j, dims=d, k_range=k, net_span=4) for j in range(1 + ci % 2)]
    assert load(h, regs) == 0, (kw, err())
    sz = [C.c_int32() for _ in range(6)]; st = C.c_int64()
    assert L.xr_batch_sizes(h, *[C.byref(s) for s in sz], C.byref(st)) == 0
    k_max = sz[3].value
    cut = bool(kw.get("force_scratch_field") or kw.get("stream_per_region"))
    base_live, base_launches = live.value, launches.value
    for trial in range(300):
        G = int(rng.integers(1, min(B, 8) + 1))
        cuts = np.sort(rng.choice(np.arange(1, B), G - 1, replace=False)) if G > 1 else np.zeros(0, np.int64)
        bounds = np.concatenate([[0], cuts, [B]]).astype(np.int32)
        assert L.xr_batch_set_groups(h, bounds.ctypes.data, G) == 0
        # bad group: XR_ERR_INVALID whatever else is wrong
        for g_bad in (-2, G, G + int(rng.integers(0, 1000)), -(1 << 31), (1 << 31) - 1):
            assert L.xr_batch_lookahead(h, g_bad, None, p, int(rng.integers(-3, k_max + 3)), None, None) == X.XR_ERR_INVALID, g_bad
            assert "group" in err()
        g = int(rng.integers(-1, G))
        assert L.xr_batch_lookahead(h, g, None, None, k_max, p, None) == X.XR_ERR_INVALID
        # k_cap too small: XR_ERR_RANGE
        if k_max > 0:
            for kc in (k_max - 1, 0, -1, -(1 << 31), int(rng.integers(-100, k_max))):
                assert L.xr_batch_lookahead(h, g, p, p, kc, p, None) == X.XR_ERR_RANGE, kc
                assert "k_cap" in err()
        # valid arguments: the documented cut, else "kernels not linked" — after every check, before any allocation or launch
        rc = L.xr_batch_lookahead(h, g, p if trial % 2 else None, p, k_max + int(rng.integers(0, 5)), p if trial % 3 else None, None)
        if cut:
            assert rc == X.XR_ERR_RANGE and "HBM scratch" in err(), (kw, rc, err())
        else:
            assert rc == X.XR_ERR_STATE and "not linked" in err(), (kw, rc, err())
        n_checked += 1
    assert (live.value, launches.value) == (base_live, base_launches), "a refused lookahead allocated or launched"
    act = np.ones(B, np.int32)
    assert L.xr_batch_step(h, act.ctypes.data, None) == 0          # the batch is as usable as before
    L.xr_batch_destroy(h)
    assert live.value == 0, ("leaked device bytes", live.value, kw)
print("HOSTSAN_LOOKAHEAD_OK", n_checked)
