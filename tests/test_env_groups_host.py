"""Env groups (xr_batch_set_groups / _step_group / _random_actions_group / _fetch_group) without a GPU: the entry points exist and refuse
null arguments with a status, the Python-side partition checks of RegionBatch / XRouteVectorEnv, and the host C++ of the four entry
points under ASan + UBSan with a few thousand hostile partitions, groups, strides and sizes (tests/hostsan/drive_groups.py)."""
import os
import subprocess
import sys

import pytest

from xroute_env_amd import _lib
from xroute_env_amd.batch import partition_bounds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP_SYMBOLS = ("xr_batch_set_groups", "xr_batch_step_group", "xr_batch_random_actions_group", "xr_batch_fetch_group")


def test_group_symbols_bound_and_exported():
    L = _lib.lib()
    for name in GROUP_SYMBOLS:
        assert name in _lib.SYMBOLS
        assert hasattr(L, name)
    assert (_lib.XR_MAX_GROUPS, _lib.XR_GROUP_INPLACE) == (64, 1)
    hdr = open(os.path.join(ROOT, "include", "xroute_hip.h")).read()
    assert "#define XR_MAX_GROUPS 64" in hdr and "#define XR_GROUP_INPLACE 1" in hdr
    for name in GROUP_SYMBOLS:
        assert name + "(" in hdr


def test_group_argument_errors_without_gpu():
    L = _lib.lib()
    assert L.xr_batch_set_groups(None, None, 1) == _lib.XR_ERR_INVALID
    assert b"null" in L.xr_last_error()
    assert L.xr_batch_step_group(None, 0, None, None, 0, 0, None) == _lib.XR_ERR_INVALID
    assert L.xr_batch_random_actions_group(None, 0, None, 1, None) == _lib.XR_ERR_INVALID
    assert L.xr_batch_fetch_group(None, 0, _lib.XR_FETCH_HASH, None, 0, None) == _lib.XR_ERR_INVALID
    assert b"xr_batch_fetch_group" in L.xr_last_error()


def test_partition_bounds():
    assert partition_bounds(1, 10) == [0, 10]
    assert partition_bounds(4, 10) == [0, 2, 5, 7, 10]
    assert partition_bounds(4, 4096) == [0, 1024, 2048, 3072, 4096]
    assert partition_bounds([0, 1, 9, 10], 10) == [0, 1, 9, 10]
    assert partition_bounds(64, 64) == list(range(65))
    for bad in (0, -1, 11, 65, True):
        with pytest.raises(ValueError):
            partition_bounds(bad, 10 if bad != 65 else 100)
    for bad in ([0], [], [1, 10], [0, 9], [0, 5, 5, 10], [0, 6, 5, 10], [0, 11, 10], list(range(66))):
        with pytest.raises(ValueError):
            partition_bounds(bad, 10 if len(bad) < 60 else 65)


def test_region_batch_group_methods_validate_before_the_library():
    """RegionBatch's group methods check their arguments like step() does; exercised here on an object that has no batch behind it
    (nothing may reach the library when a check fails)."""
    import torch
    from xroute_env_amd.batch import RegionBatch
    rb = RegionBatch.__new__(RegionBatch)
    rb.n_envs, rb.device, rb.legal_words, rb.path_cap, rb.n_max = 10, torch.device("cpu"), 1, 8, 16
    assert rb.n_groups == 1 and rb.group_bounds(0) == (0, 10)
    rb._group_bounds = [0, 3, 10]
    assert rb.n_groups == 2 and rb.group_bounds(1) == (3, 10)
    for g in (-1, 2, 99):
        with pytest.raises(ValueError):
            rb.group_bounds(g)
    with pytest.raises(ValueError, match="group's size"):
        rb.step_group(0, torch.zeros(10, dtype=torch.int32))
    with pytest.raises(ValueError, match="group's size"):
        rb.step_group(1, torch.zeros(7, dtype=torch.int64))
    with pytest.raises(ValueError, match="per-env"):
        rb.fetch_group("steps", 0)
    with pytest.raises(ValueError, match="per-env"):
        rb.fetch_group("route_order", 0)
    with pytest.raises(ValueError):
        rb.set_groups([0, 5, 5, 10])


def test_vector_env_group_calls_need_groups():
    from xroute_env_amd.envs.vector_env import XRouteVectorEnv
    env = XRouteVectorEnv.__new__(XRouteVectorEnv)
    env.n_groups = 0
    with pytest.raises(RuntimeError, match="groups="):
        env.step_wait()
    with pytest.raises(RuntimeError, match="groups="):
        env.poll(0)
    env.n_groups = 3
    with pytest.raises(ValueError):
        env._groups_of(3)
    assert list(env._groups_of(None)) == [0, 1, 2] and env._groups_of(2) == (2,)


def _asan_env():
    libasan = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(libasan) or not os.path.exists(libasan):
        pytest.skip("libasan not found")
    return dict(os.environ, LD_PRELOAD=libasan, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def test_group_host_code_under_asan_ubsan():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "hostsan"), "libxr_host_asan.so"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail("sanitizer build of the host code failed: " + r.stderr[-1500:])
    so = os.path.join(ROOT, "tests", "hostsan", "libxr_host_asan.so")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hostsan", "drive_groups.py"), ROOT, so], capture_output=True, text=True,
                         env=_asan_env(), timeout=900)
    assert out.returncode == 0 and "HOSTSAN_GROUPS_OK" in out.stdout, (out.stdout[-800:], out.stderr[-5000:])
