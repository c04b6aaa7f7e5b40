"""Rollouts (xr_batch_rollout) without a GPU: the entry point is exported, bound with its argument types and declared in the header with
its three constants; _lib.rollout_seed is the documented seed_r; RegionBatch.rollout / XRouteVectorEnv check their arguments before the
library; and the validators of the host C++ run under ASan + UBSan as a program of their own (tests/hostsan_rollout/rollout_args.cpp)."""
import ctypes as C
import os
import subprocess

import pytest

from xroute_env_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSAN = os.path.join(ROOT, "tests", "hostsan_rollout")


def test_rollout_symbol_bound_and_declared():
    L = _lib.lib()
    assert "xr_batch_rollout" in _lib.SYMBOLS and hasattr(L, "xr_batch_rollout")
    vp, i32 = C.c_void_p, C.c_int32
    assert list(L.xr_batch_rollout.argtypes) == [vp, i32, i32, i32, C.c_uint64, vp, i32, i32, vp, vp, vp, vp, i32, vp]
    assert L.xr_batch_rollout.restype is C.c_int32
    hdr = open(os.path.join(ROOT, "include", "xroute_hip.h")).read()
    assert "int32_t xr_batch_rollout(xr_batch* b, int32_t group, int32_t n_rollouts, int32_t policy, uint64_t seed," in hdr
    assert "#define XR_ABI_VERSION 9" in hdr and L.xr_abi_version() == 9          # an addition: the ABI version stays
    for name, value in (("XR_ROLLOUT_STOP", 0), ("XR_ROLLOUT_RANDOM", 1), ("XR_ROLLOUT_MAX", 4096)):
        assert getattr(_lib, name) == value
        assert any(l.split()[:3] == ["#define", name, str(value)] for l in hdr.splitlines()), name
    # the contract the header must state
    for phrase in ("never synchronises", "NO TRACE", "0x9E3779B97F4A7C15", "XR_ENV_BAD_ACTION", "costs no ply", "auto-reset", "stream_per_region",
                   "first call", "claim counters of its own", "ordered by the caller"):
        assert phrase in hdr[hdr.index("---- rollouts"):], phrase


def test_rollout_seed_is_the_documented_formula_mod_2_64():
    g = 0x9E3779B97F4A7C15
    assert _lib.rollout_seed(12345, 0) == 12345
    assert _lib.rollout_seed(0, 1) == g
    assert _lib.rollout_seed(2 ** 64 - 1, 1) == g - 1                      # wraps
    assert _lib.rollout_seed(7, 3) == (7 + 3 * g) % 2 ** 64 and 3 * g > 2 ** 64
    assert all(0 <= _lib.rollout_seed(s, r) < 2 ** 64 for s in (0, 2 ** 63, 2 ** 64 - 1) for r in (0, 1, 4095))
    assert _lib.rollout_seed(2 ** 64 + 5, 2) == _lib.rollout_seed(5, 2)


def test_rollout_null_arguments_without_gpu():
    L = _lib.lib()
    assert L.xr_batch_rollout(None, -1, 1, 1, 0, None, 0, 0, None, None, None, None, 0, None) == _lib.XR_ERR_INVALID
    msg = L.xr_last_error()
    assert b"xr_batch_rollout" in msg and b"null" in msg
    out = (C.c_int32 * 16)()
    assert L.xr_batch_rollout(None, 0, 2, 1, 0, None, 0, 0, out, None, None, None, 0, None) == _lib.XR_ERR_INVALID


def test_product_library_links_the_rollout_kernel():
    """The launcher is weak in csrc/xr_device.h (so that the host-only sanitizer build links): the product library must define it."""
    assert hasattr(_lib.lib(), "xr_launch_line")          # (the rollout: kind XR_LINE_POLICY of the one line launcher)


def test_region_batch_rollout_validates_before_the_library():
    import torch
    from xroute_env_amd.batch import RegionBatch
    rb = RegionBatch.__new__(RegionBatch)
    rb.n_envs, rb.device, rb.legal_words, rb.k_max = 10, torch.device("cpu"), 1, 5
    rb._group_bounds = [0, 3, 10]
    bufs = dict(out=torch.zeros((10, 2, 8), dtype=torch.int32), return_out=torch.zeros((10, 2), dtype=torch.float64),
                hash_out=torch.zeros((10, 2), dtype=torch.int64), order_out=torch.zeros((10, 2, 5), dtype=torch.int32))
    with pytest.raises(ValueError):
        rb.rollout(2, group=2)
    for bad in (0, -1, _lib.XR_ROLLOUT_MAX + 1):
        with pytest.raises(ValueError, match="n_rollouts"):
            rb.rollout(bad, **bufs)
    for bad in ("greedy", 2, -1, True):
        with pytest.raises(ValueError, match="policy"):
            rb.rollout(2, policy=bad, **bufs)
    with pytest.raises(ValueError, match="max_plies"):
        rb.rollout(2, max_plies=-1, **bufs)
    with pytest.raises(ValueError, match="out must"):
        rb.rollout(2, **dict(bufs, out=bufs["out"].to(torch.int64)))
    with pytest.raises(ValueError, match="out must"):
        rb.rollout(2, group=1, **bufs)                                       # (the group has 7 rows)
    with pytest.raises(ValueError, match="return_out"):
        rb.rollout(2, **dict(bufs, return_out=bufs["return_out"].to(torch.float32)))
    with pytest.raises(ValueError, match="hash_out"):
        rb.rollout(2, **dict(bufs, hash_out=torch.zeros((10, 3), dtype=torch.int64)))
    with pytest.raises(ValueError, match="order_out"):
        rb.rollout(2, **dict(bufs, order_out=torch.zeros((10, 2, 4), dtype=torch.int32)))
    for bad in (torch.zeros((10, 2, 3), dtype=torch.int64), torch.zeros((10, 3, 3), dtype=torch.int32), torch.zeros((10, 2), dtype=torch.int32),
                torch.zeros((10, 2, 0), dtype=torch.int32), torch.zeros((10, 2, 6), dtype=torch.int32)[:, :, ::2]):
        with pytest.raises(ValueError, match="prefix"):
            rb.rollout(2, prefix=bad, **bufs)


def test_first_of_best_takes_the_first_maximum_and_zero_for_a_done_env():
    import torch
    from xroute_env_amd.envs.vector_env import XRouteVectorEnv
    ret = torch.tensor([[-3.0, -1.0, -1.0], [0.0, 0.0, 0.0], [-2.0, -5.0, -2.0], [-9.0, -8.0, -7.5]], dtype=torch.float64)
    order = torch.tensor([[[4, 1], [2, 1], [3, 1]], [[0, 0], [0, 0], [0, 0]], [[5, 2], [6, 2], [7, 2]], [[1, 2], [2, 1], [3, 1]]], dtype=torch.int32)
    act = XRouteVectorEnv._first_of_best({"ret": ret, "order": order})
    assert act.dtype == torch.int32 and act.tolist() == [2, 0, 5, 3]


def test_rollout_host_code_under_asan_ubsan_as_a_program_of_its_own():
    r = subprocess.run(["make", "-C", HOSTSAN, "rollout_args"], capture_output=True, text=True)
    assert r.returncode == 0, "build of the rollout argument program failed: " + r.stderr[-1500:]
    assert "warning" not in r.stderr, r.stderr[-1500:]
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([os.path.join(HOSTSAN, "rollout_args")], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("ROLLOUT_ARGS_OK "), (out.stdout[-1500:], out.stderr[-3000:])
    assert out.stderr == "", out.stderr[-3000:]
