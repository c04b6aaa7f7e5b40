"""Tree search (xr_batch_tree_search, XR-Tree v1) without a GPU: the entry points are exported, bound with their argument types and
declared in the header in their place; the exploration table of the library against Python's math; RegionBatch.tree_search checks its
arguments before the library; the spec's twin (tests/tree_twin.py) on hand-made returns; and the validators of the host C++ under ASan +
UBSan as a program of their own (tests/hostsan_tree/tree_args.cpp)."""
import ctypes as C
import math
import os
import subprocess

import pytest

from tests import tree_twin
from xroute_env_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSAN = os.path.join(ROOT, "tests", "hostsan_tree")
INF = float("inf")


def test_tree_symbols_bound_and_declared():
    L = _lib.lib()
    vp, i32, f64 = C.c_void_p, C.c_int32, C.c_double
    for name in ("xr_batch_tree_search", "xr_tree_exploration_table"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
        assert getattr(L, name).restype is i32
    assert list(L.xr_batch_tree_search.argtypes) == [vp, i32, i32, i32, C.c_uint64, vp, i32, f64, f64, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    assert list(L.xr_tree_exploration_table.argtypes) == [f64, f64, i32, vp]
    hdr = open(os.path.join(ROOT, "include", "xroute_hip.h")).read()
    assert "int32_t xr_batch_tree_search(xr_batch* b, int32_t group, int32_t n_waves, int32_t n_par, uint64_t seed," in hdr
    assert "int32_t xr_tree_exploration_table(double c_init, double c_base, int32_t n, double* out_host);" in hdr
    assert "#define XR_ABI_VERSION 9" in hdr and L.xr_abi_version() == 9          # an addition: the ABI version stays
    assert _lib.XR_TREE_POOL_FULL == 1
    assert any(l.split()[:3] == ["#define", "XR_TREE_POOL_FULL", "1"] for l in hdr.splitlines())
    # the section is in its place
    assert hdr.index("---- branch") < hdr.index("---- tree search") < hdr.index("---- XR-Maze v2: global-route guides")
    sec = hdr[hdr.index("---- tree search"):hdr.index("---- XR-Maze v2: global-route guides")]
    for phrase in ("XR-Tree v1", "never synchronises", "NO TRACE", "first call", "40 node_cap", "shadow slots", "in-place observation",
                   "DIFFERENT groups", "ordered by the caller", "0xD1B54A32D192ED03", "XR_TREE_POOL_FULL", "lowest", "auto-reset",
                   "stream_per_region", "XR_ERR_NOMEM", "no tree reuse", "Dirichlet"):
        assert phrase in sec, phrase


def test_tree_seed_is_the_documented_formula_mod_2_64():
    g = 0xD1B54A32D192ED03
    assert _lib.tree_seed(5, 0) == 5 and _lib.tree_seed(0, 1) == g
    assert _lib.tree_seed(2 ** 64 - 1, 1) == g - 1
    assert _lib.tree_seed(7, 3) == (7 + 3 * g) % 2 ** 64


def test_tree_null_arguments_without_gpu():
    L = _lib.lib()
    args = (-1, 2, 2, 0, None, 8, 1.25, 19652.0)
    assert L.xr_batch_tree_search(None, *args, None, None, 4, None, None, None, None, None, None) == _lib.XR_ERR_INVALID
    msg = L.xr_last_error()
    assert b"xr_batch_tree_search" in msg and b"null" in msg
    v, val, info = (C.c_int32 * 16)(), (C.c_double * 16)(), (C.c_int32 * 16)()
    assert L.xr_batch_tree_search(None, *args, v, val, 4, info, None, None, None, None, None) == _lib.XR_ERR_INVALID
    assert L.xr_tree_exploration_table(1.25, 19652.0, 4, None) == _lib.XR_ERR_INVALID
    assert b"xr_tree_exploration_table" in L.xr_last_error()
    out = (C.c_double * 5)()
    for bad in ((float("nan"), 19652.0, 4), (1.25, 0.0, 4), (1.25, -1.0, 4), (1.25, 19652.0, -1)):
        assert L.xr_tree_exploration_table(*bad, out) == _lib.XR_ERR_INVALID, bad


def test_product_library_links_the_tree_kernels():
    """The launchers are weak in csrc/xr_device.h (so that the host-only sanitizer build links): the product library must define them."""
    for name in ("xr_launch_tree_reset", "xr_launch_tree_select", "xr_launch_tree_backup"):
        assert hasattr(_lib.lib(), name), name


def _ulps(a, b):
    if a == b:
        return 0
    import struct
    ia, ib = (struct.unpack("<q", struct.pack("<d", x))[0] for x in (a, b))
    return abs(ia - ib)


def test_exploration_table_against_python_math():
    tabs = []
    for c_init, c_base in ((1.25, 19652.0), (0.3, 7.0)):
        n = 4096
        E = _lib.tree_exploration_table(c_init, c_base, n)
        assert len(E) == n + 1 and E[0] == 0.0
        for i in range(n + 1):
            want = (math.log((i + c_base + 1) / c_base) + c_init) * math.sqrt(i)
            assert _ulps(E[i], want) <= 2, (c_init, c_base, i, E[i], want)
        assert all(b > a for a, b in zip(E, E[1:])), "monotone"
        tabs.append(E)
    assert tabs[0] != tabs[1]
    assert _lib.tree_exploration_table(1.25, 19652.0, 0) == [0.0]


def test_region_batch_tree_search_validates_before_the_library():
    import torch
    from xroute_env_amd.batch import RegionBatch
    rb = RegionBatch.__new__(RegionBatch)          # no handle, no library: whatever gets past the checks fails on the missing attributes
    rb.n_envs, rb.device, rb.legal_words, rb.k_max = 10, torch.device("cpu"), 1, 5
    rb._group_bounds = [0, 3, 10]
    with pytest.raises(ValueError):
        rb.tree_search(2, 2, group=2)
    for bad in (0, -1):
        with pytest.raises(ValueError, match="n_waves"):
            rb.tree_search(bad, 2)
    for bad in (0, -1, _lib.XR_ROLLOUT_MAX + 1):
        with pytest.raises(ValueError, match="n_par"):
            rb.tree_search(2, bad)
    with pytest.raises(ValueError, match="n_waves x n_par"):
        rb.tree_search(17, 4096)
    for bad in (float("nan"), INF, -INF):
        with pytest.raises(ValueError, match="c_init"):
            rb.tree_search(2, 2, c_init=bad)
    for bad in (0.0, -3.0, float("nan"), INF):
        with pytest.raises(ValueError, match="c_base"):
            rb.tree_search(2, 2, c_base=bad)
    for bad in (0, -4, 2 ** 31):
        with pytest.raises(ValueError, match="node_cap"):
            rb.tree_search(2, 2, node_cap=bad)
    for bad in (torch.zeros((10, 5), dtype=torch.float64), torch.zeros((10, 4)), torch.zeros((9, 5)), torch.zeros((10, 10))[:, ::2], [[0.0] * 5] * 10):
        with pytest.raises(ValueError, match="prior"):
            rb.tree_search(2, 2, prior=bad)
    with pytest.raises(ValueError, match="prior"):
        rb.tree_search(2, 2, prior=torch.zeros((10, 5)), group=1)          # (the group has 7 rows)


# ---- the twin on hand-made returns -------------------------------------------------------------------------------------------------
def _E(n, c_init=1.25, c_base=19652.0):
    return _lib.tree_exploration_table(c_init, c_base, n)


def _run(legal, n_waves, n_par, node_cap, value, prior=None, k_cap=None):
    """value(path) -> G of a simulation whose path is `path`; the order of a simulation: its path, then the other nets ascending."""
    k_cap = k_cap or max(legal, default=1)

    def evaluate(w, paths):
        rets = [[value(tuple(p)) for p in row] for row in paths]
        orders = [[list(p) + [n for n in sorted(legal) if n not in p] for p in row] for row in paths]
        return rets, orders
    res, paths, returns, trees = tree_twin.search([legal], n_waves, n_par, node_cap, _E(n_waves * n_par), evaluate, k_cap,
                                                  None if prior is None else [prior])
    return res[0], paths[0], returns[0], trees[0]


def test_twin_ties_go_to_the_lowest_net():
    # the root is expanded at the start, every child scores 0 (E[0] == 0): the lowest net wins, and the lane stops at that unexpanded child
    res, paths, _, tree = _run([2, 3, 5], 1, 1, 100, lambda p: -1.0)
    assert paths[0] == [2, 0, 0, 0, 0] and tree.ties == 1
    assert res["visits"] == [0, 1, 0, 0, 0] and res["value"][1] == -1.0 and res["value"][0] == -INF
    assert res["info"] == [1, 1 + 3 + 2, 1, 0]


def test_twin_pending_visits_spread_the_lanes_of_one_wave():
    # wave 0: nothing is backed up while the lanes select, only V tells them apart — three lanes take three different children
    res, paths, _, tree = _run([1, 2, 3], 1, 3, 100, lambda p: -float(p[0]))
    assert [p[0] for p in paths] == [1, 2, 3]
    assert res["visits"] == [1, 1, 1] and res["value"] == [-1.0, -2.0, -3.0]
    assert all(n.V == 0 for n in tree.nodes) and tree.nodes[0].N == 3
    # a fourth lane meets three children with one pending visit each: a tie again, net 1, now expanded: it goes one level down
    _, paths, _, _ = _run([1, 2, 3], 1, 4, 100, lambda p: -1.0)
    assert paths[3][:2] == [1, 2]


def test_twin_min_equal_max_gives_v_zero():
    # every return is the same: max == min, v stays 0 and the search is the prior's and the visit counts' alone
    seen = []

    def value(p):
        seen.append(p)
        return -7.5
    res, paths, returns, tree = _run([1, 2], 6, 1, 100, value)
    assert tree.mn == tree.mx == -7.5 and set(returns) == {-7.5}
    assert res["visits"] == [3, 3]          # u alone: the less visited child, ties to net 1
    assert res["value"] == [-7.5, -7.5] and res["best_return"] == -7.5 and res["best_order"] == [1, 2]
    # with a spread, the better child takes the visits
    res, _, _, _ = _run([1, 2], 6, 1, 100, lambda p: -1.0 if p[:1] == (2,) else -100.0)
    assert res["visits"][1] > res["visits"][0] and res["best_order"] == [2, 1] and res["best_return"] == -1.0


def test_twin_pool_too_small_for_the_root():
    for cap in (1, 3):
        res, paths, _, tree = _run([1, 2, 3], 2, 2, cap, lambda p: -1.0)
        assert all(p == [0, 0, 0] for p in paths) and len(paths) == 4
        assert res["info"] == [4, 1, 0, tree_twin.POOL_FULL] and res["visits"] == [0, 0, 0] and res["value"] == [-INF] * 3
        assert tree.nodes[0].N == 4 and tree.nodes[0].V == 0
        assert res["best_order"] == [1, 2, 3] and res["best_return"] == -1.0


def test_twin_pool_too_small_for_a_grandchild():
    # 1 + 3 fits, a child's block of 2 does not: every path has one net, the flag is set, the visits still spread
    res, paths, _, _ = _run([1, 2, 3], 3, 2, 5, lambda p: -float(p[0]))
    assert all(p[0] > 0 and p[1:] == [0, 0] for p in paths)
    assert res["info"][1:] == [4, 1, tree_twin.POOL_FULL] and sum(res["visits"]) == 6
    # one more block fits, the next does not
    res, paths, _, _ = _run([1, 2, 3], 4, 2, 6, lambda p: -float(p[0]))
    assert res["info"][1:] == [6, 2, tree_twin.POOL_FULL]


def test_twin_terminal_nodes():
    # one net: the root's only child is terminal, every simulation ends there and nothing more is allocated
    res, paths, _, tree = _run([4], 2, 2, 100, lambda p: -2.0, k_cap=4)
    assert all(p == [4, 0, 0, 0] for p in paths) and tree.terminal_visits == 4
    assert res["info"] == [4, 2, 1, 0] and res["visits"] == [0, 0, 0, 4] and res["value"][3] == -2.0
    # two nets: terminal at depth 2
    res, paths, _, tree = _run([1, 2], 4, 2, 100, lambda p: -1.0)
    assert tree.terminal_visits > 0 and res["info"][2] == 2 and res["info"][1] == 1 + 2 + 1 + 1
    # no net: a done row
    res, paths, returns, tree = _run([], 2, 2, 100, lambda p: 0.0, k_cap=3)
    assert res == dict(visits=[0, 0, 0], value=[-INF] * 3, info=[0, 0, 0, 0], best_order=[0, 0, 0], best_return=-INF)
    assert paths == [[0, 0, 0]] * 4 and returns == [0.0] * 4


def test_twin_prior_zero_sum_is_uniform_and_bad_entries_count_as_zero():
    _, _, _, t0 = _run([1, 2, 3], 1, 1, 100, lambda p: -1.0, prior=[0.0, 0.0, 0.0])
    assert [t0.nodes[i].P for i in (1, 2, 3)] == [1.0 / 3.0] * 3
    _, _, _, t1 = _run([1, 2, 3], 1, 1, 100, lambda p: -1.0, prior=[float("nan"), -4.0, INF])
    assert [t1.nodes[i].P for i in (1, 2, 3)] == [1.0 / 3.0] * 3
    _, paths, _, t2 = _run([1, 2, 3], 1, 2, 100, lambda p: -1.0, prior=[1.0, float("nan"), 3.0])
    assert [t2.nodes[i].P for i in (1, 2, 3)] == [0.25, 0.0, 0.75]
    # a child's block normalises over ITS legal nets: below net 1 the nets 2 and 3 remain, 0 + 3
    first = t2.nodes[1].first
    assert first > 0 and [t2.nodes[first + i].P for i in (0, 1)] == [0.0, 1.0]
    # the prior decides once E is not 0: wave 1's first lane meets the root at n = 1 and takes the heavier net
    _, paths, _, _ = _run([1, 2, 3], 2, 1, 100, lambda p: -1.0, prior=[1.0, 0.0, 3.0])
    assert paths[0][0] == 1 and paths[1][0] == 3


def test_tree_host_code_under_asan_ubsan_as_a_program_of_its_own():
    r = subprocess.run(["make", "-C", HOSTSAN, "tree_args"], capture_output=True, text=True)
    assert r.returncode == 0, "build of the tree argument program failed: " + r.stderr[-1500:]
    assert "warning" not in r.stderr, r.stderr[-1500:]
    out = subprocess.run([os.path.join(HOSTSAN, "tree_args")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("TREE_ARGS_OK "), (out.stdout[-1500:], out.stderr[-3000:])
    assert out.stderr == "", out.stderr[-3000:]
