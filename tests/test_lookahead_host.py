"""Lookahead (xr_batch_lookahead) without a GPU: the entry point is exported, bound with its argument types and declared in the header;
it refuses a null batch with a status and a message; RegionBatch.lookahead / XRouteVectorEnv check their arguments before the library;
and the validators of the host C++ run under ASan + UBSan (tests/hostsan/drive_lookahead.py)."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from xroute_env_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lookahead_symbol_bound_and_declared():
    L = _lib.lib()
    assert "xr_batch_lookahead" in _lib.SYMBOLS and hasattr(L, "xr_batch_lookahead")
    vp = C.c_void_p
    assert list(L.xr_batch_lookahead.argtypes) == [vp, C.c_int32, vp, vp, C.c_int32, vp, vp]
    assert L.xr_batch_lookahead.restype is C.c_int32
    hdr = open(os.path.join(ROOT, "include", "xroute_hip.h")).read()
    assert "int32_t xr_batch_lookahead(xr_batch* b, int32_t group, const uint64_t* cand_mask_dev," in hdr
    assert "#define XR_ABI_VERSION 9" in hdr and L.xr_abi_version() == 9          # an addition: the ABI version stays
    # the contract the header must state
    for phrase in ("never synchronises", "NO TRACE", "{0, 0, 0, -1}", "-inf", "HBM-scratch", "stream_per_region", "first call"):
        assert phrase in hdr, phrase


def test_lookahead_null_arguments_without_gpu():
    L = _lib.lib()
    assert L.xr_batch_lookahead(None, -1, None, None, 0, None, None) == _lib.XR_ERR_INVALID
    msg = L.xr_last_error()
    assert b"xr_batch_lookahead" in msg and b"null" in msg
    out = (C.c_int32 * 16)()
    assert L.xr_batch_lookahead(None, 0, None, out, 4, None, None) == _lib.XR_ERR_INVALID


def test_product_library_links_the_lookahead_kernels():
    """The launchers are weak in csrc/xr_device.h (so that the host-only sanitizer build links): the product library must define them."""
    L = _lib.lib()
    for name in ("xr_launch_lookahead", "xr_launch_lookahead_plan", "xr_lookahead_occupancy"):
        assert hasattr(L, name), name


def test_region_batch_lookahead_validates_before_the_library():
    import torch
    from xroute_env_amd.batch import RegionBatch
    rb = RegionBatch.__new__(RegionBatch)
    rb.n_envs, rb.device, rb.legal_words, rb.k_max = 10, torch.device("cpu"), 1, 5
    rb._group_bounds = [0, 3, 10]
    with pytest.raises(ValueError):
        rb.lookahead(group=2)
    with pytest.raises(ValueError, match="int32"):
        rb.lookahead(out=torch.zeros((10, 5, 4), dtype=torch.int64), reward_out=torch.zeros((10, 5), dtype=torch.float64))
    with pytest.raises(ValueError, match="int32"):
        rb.lookahead(out=torch.zeros((10, 5, 4), dtype=torch.int32), reward_out=torch.zeros((10, 5), dtype=torch.float64), group=1)
    with pytest.raises(ValueError, match="float64"):
        rb.lookahead(out=torch.zeros((10, 5, 4), dtype=torch.int32), reward_out=torch.zeros((10, 5), dtype=torch.float32))
    with pytest.raises(ValueError, match="mask"):
        rb.lookahead(out=torch.zeros((7, 5, 4), dtype=torch.int32), reward_out=torch.zeros((7, 5), dtype=torch.float64), group=1,
                     mask=torch.zeros((7, 2), dtype=torch.int64))


def test_argmax_first_is_the_first_maximum_and_zero_without_candidates():
    import torch
    from xroute_env_amd.envs.vector_env import XRouteVectorEnv
    ninf = float("-inf")
    r = torch.tensor([[ninf, -3.0, -1.0, -1.0], [ninf, ninf, ninf, ninf], [-2.0, -2.0, ninf, -5.0], [ninf, ninf, ninf, -0.0]], dtype=torch.float64)
    act = XRouteVectorEnv._argmax_first(r)
    assert act.dtype == torch.int32 and act.tolist() == [3, 0, 1, 4]


def _asan_env():
    libasan = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(libasan) or not os.path.exists(libasan):
        pytest.skip("libasan not found")
    return dict(os.environ, LD_PRELOAD=libasan, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def test_lookahead_host_code_under_asan_ubsan():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "hostsan"), "libxr_host_asan.so"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail("sanitizer build of the host code failed: " + r.stderr[-1500:])
    so = os.path.join(ROOT, "tests", "hostsan", "libxr_host_asan.so")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hostsan", "drive_lookahead.py"), ROOT, so], capture_output=True, text=True,
                         env=_asan_env(), timeout=900)
    assert out.returncode == 0 and "HOSTSAN_LOOKAHEAD_OK" in out.stdout, (out.stdout[-800:], out.stderr[-5000:])
