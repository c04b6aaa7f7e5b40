"""Branch (xr_batch_branch) without a GPU: the entry point is exported, bound with its argument types and declared in the header with the
contract it must state; null arguments are refused; the product library links the kernels; RegionBatch.branch checks its map before the
library; the beam selection rule as a pure function on hand-made tables; and the validators of the host C++ run under ASan + UBSan as a
program of their own (tests/hostsan_branch/branch_args.cpp)."""
import ctypes as C
import os
import subprocess

import pytest

from xroute_env_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSAN = os.path.join(ROOT, "tests", "hostsan_branch")
INF = float("inf")


def test_branch_symbol_bound_and_declared():
    L = _lib.lib()
    assert "xr_batch_branch" in _lib.SYMBOLS and hasattr(L, "xr_batch_branch")
    vp, i32 = C.c_void_p, C.c_int32
    assert list(L.xr_batch_branch.argtypes) == [vp, i32, vp, vp]
    assert L.xr_batch_branch.restype is C.c_int32
    hdr = open(os.path.join(ROOT, "include", "xroute_hip.h")).read()
    assert "int32_t xr_batch_branch(xr_batch* b, int32_t group, const int32_t* parent_dev, void* stream);" in hdr
    assert "#define XR_ABI_VERSION 9" in hdr and L.xr_abi_version() == 9          # an addition: the ABI version stays
    assert hdr.index("---- rollouts") < hdr.index("---- branch") < hdr.index("---- XR-Maze v2: global-route guides")
    section = hdr[hdr.index("---- branch"):hdr.index("---- XR-Maze v2: global-route guides")]
    # the contract the header must state
    for phrase in ("Gather semantics", "BEFORE the call", "never synchronises", "XR_ENV_BAD_ACTION", "parent[i] >= rows", "validity is dropped",
                   "every router variant", "HBM-scratch", "stream_per_region", "first call", "bytes", "byte-identical", "need not be injective",
                   "ordered by the caller", "XR_ERR_INVALID", "XR_ERR_STATE"):
        assert phrase in section, phrase


def test_branch_null_arguments_without_gpu():
    L = _lib.lib()
    parent = (C.c_int32 * 4)(0, 1, 2, 3)
    for args in ((None, -1, None, None), (None, -1, parent, None), (None, 0, parent, None)):
        assert L.xr_batch_branch(*args) == _lib.XR_ERR_INVALID
        msg = L.xr_last_error()
        assert b"xr_batch_branch" in msg and b"null" in msg


def test_product_library_links_the_branch_kernels():
    """The launcher is weak in csrc/xr_device.h (so that the host-only sanitizer build links): the product library must define it."""
    assert hasattr(_lib.lib(), "xr_launch_branch")


def test_region_batch_branch_validates_before_the_library():
    import torch
    from xroute_env_amd.batch import RegionBatch

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError(f"the library was reached ({name})")

    rb = RegionBatch.__new__(RegionBatch)
    rb.n_envs, rb.device, rb.legal_words, rb.k_max = 10, torch.device("cpu"), 1, 5
    rb._group_bounds = [0, 3, 10]
    rb.L, rb._h, rb.region_epoch = NoLibrary(), None, 0
    good = torch.arange(10, dtype=torch.int32)
    for bad in (good.to(torch.int64), good.to(torch.int16), good.to(torch.float32),                    # wrong dtype
                good[:9].contiguous(), torch.arange(11, dtype=torch.int32), good.view(2, 5), good.view(10, 1),      # wrong length / shape
                torch.arange(20, dtype=torch.int32)[::2],                                              # non-contiguous
                good.tolist()):                                                                        # not a tensor
        with pytest.raises(ValueError, match="parent must"):
            rb.branch(bad)
    for g, rows in ((0, 3), (1, 7)):
        for n in (rows - 1, rows + 1, 10):
            if n != rows:
                with pytest.raises(ValueError, match=f"int32 \\[{rows}\\]"):
                    rb.branch(torch.zeros(n, dtype=torch.int32), group=g)
        with pytest.raises(ValueError, match="parent must"):
            rb.branch(torch.zeros(rows, dtype=torch.int64), group=g)
        with pytest.raises(ValueError, match="parent must"):
            rb.branch(torch.zeros(2 * rows, dtype=torch.int32)[::2], group=g)
    for g in (2, -1, 64):
        with pytest.raises(ValueError, match="group"):
            rb.branch(good, group=g)
    assert rb.region_epoch == 0                                    # nothing was branched


# ---- the beam selection rule ----------------------------------------------------------------------------------------------------------
def _select(rows, width):
    import torch
    from xroute_env_amd.envs.beam import select_beams
    parent, net, alive = select_beams(torch.tensor(rows, dtype=torch.float64), width)
    assert parent.dtype == torch.int64 and net.dtype == torch.int64 and alive.dtype == torch.bool
    return parent.tolist(), net.tolist(), alive.tolist()


def test_beam_selection_orders_by_value_then_parent_then_net():
    # one region, 2 beams x 3 nets
    parent, net, alive = _select([[[-5.0, -1.0, -3.0], [-2.0, -4.0, -0.5]]], 2)
    assert (parent, net, alive) == ([[1, 0]], [[3, 2]], [[True, True]])
    parent, net, alive = _select([[[-5.0, -1.0, -3.0], [-2.0, -4.0, -0.5]]], 4)
    assert (parent, net) == ([[1, 0, 1, 0]], [[3, 2, 1, 3]]) and alive == [[True] * 4]


def test_beam_selection_ties_go_to_the_lower_parent_then_the_lower_net():
    t = [[[-1.0, -2.0, -1.0], [-1.0, -1.0, -2.0], [-2.0, -1.0, -1.0]]]
    parent, net, alive = _select(t, 3)
    assert (parent, net) == ([[0, 0, 1]], [[1, 3, 1]]) and alive == [[True] * 3]
    parent, net, _ = _select(t, 6)
    assert list(zip(parent[0], net[0])) == [(0, 1), (0, 3), (1, 1), (1, 2), (2, 2), (2, 3)]
    # an all-equal table: the flat (parent, net) order
    parent, net, _ = _select([[[0.0, 0.0], [0.0, 0.0]]], 2)
    assert (parent, net) == ([[0, 0]], [[1, 2]])
    # -0.0 == 0.0: still a tie, the lower net first
    parent, net, _ = _select([[[0.0, -0.0], [-0.0, 0.0]]], 4)
    assert list(zip(parent[0], net[0])) == [(0, 1), (0, 2), (1, 1), (1, 2)]


def test_beam_selection_minus_inf_rows_are_dead_beams_and_regions_are_independent():
    t = [[[-INF, -INF, -INF], [-3.0, -INF, -1.0], [-INF, -INF, -INF]],          # one live beam, two candidates
         [[-INF, -INF, -INF]] * 3,                                                # a finished region
         [[-7.0, -8.0, -9.0], [-INF, -INF, -INF], [-7.0, -INF, -INF]]]
    parent, net, alive = _select(t, 3)
    assert parent == [[1, 1, -1], [-1, -1, -1], [0, 2, 0]]
    assert net == [[3, 1, 0], [0, 0, 0], [1, 1, 2]]
    assert alive == [[True, True, False], [False] * 3, [True] * 3]


def test_beam_selection_with_fewer_finite_candidates_than_the_width():
    parent, net, alive = _select([[[-2.0, -INF], [-INF, -1.0]]], 2)
    assert (parent, net, alive) == ([[1, 0]], [[2, 1]], [[True, True]])
    parent, net, alive = _select([[[-2.0, -INF], [-INF, -INF]]], 2)
    assert (parent, net, alive) == ([[0, -1]], [[1, 0]], [[True, False]])


def test_beam_selection_in_a_region_with_one_net():
    # k_max = 1: at ply 0 one beam is alive and has one candidate; width 4 keeps one beam, the rest are dead
    parent, net, alive = _select([[[-4.5], [-INF], [-INF], [-INF]]], 4)
    assert (parent, net, alive) == ([[0, -1, -1, -1]], [[1, 0, 0, 0]], [[True, False, False, False]])
    # a table with fewer (beam, net) pairs than the width asked for
    parent, net, alive = _select([[[-4.5]]], 3)
    assert (parent, net, alive) == ([[0, -1, -1]], [[1, 0, 0]], [[True, False, False]])
    with pytest.raises(ValueError):
        _select([[[-1.0]]], 0)
    with pytest.raises(ValueError):
        _select([[-1.0]], 1)


def test_branch_host_code_under_asan_ubsan_as_a_program_of_its_own():
    r = subprocess.run(["make", "-C", HOSTSAN, "branch_args"], capture_output=True, text=True)
    assert r.returncode == 0, "build of the branch argument program failed: " + r.stderr[-1500:]
    assert "warning" not in r.stderr, r.stderr[-1500:]
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([os.path.join(HOSTSAN, "branch_args")], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("BRANCH_ARGS_OK "), (out.stdout[-1500:], out.stderr[-3000:])
    assert out.stderr == "", out.stderr[-3000:]
