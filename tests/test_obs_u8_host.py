"""uint8 observations, host side (no GPU): the entry points are declared, bound and exported, refuse null / invalid arguments without
touching a device, and the fixed-shape spaces take a uint8 grid."""
import ctypes as C
import os
import re

import numpy as np

from xroute_env_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("xr_batch_step_observe_u8", "xr_batch_observation_u8")


def test_u8_symbols_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "xroute_hip.h")).read()
    assert re.search(r"#define\s+XR_OBS_U8_INPLACE\s+1\b", text) and _lib.XR_OBS_U8_INPLACE == 1
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SYMBOLS
        assert hasattr(L, name) and getattr(L, name).argtypes
    assert L.xr_abi_version() == 9


def test_u8_null_and_invalid_arguments_refused_without_a_device():
    L = _lib.lib()
    buf = (C.c_uint8 * 64)()
    acts = (C.c_int32 * 4)()
    assert L.xr_batch_step_observe_u8(None, -1, acts, buf, 16, 0, None) == _lib.XR_ERR_INVALID
    assert L.xr_batch_step_observe_u8(None, -1, None, None, 16, 0, None) == _lib.XR_ERR_INVALID
    assert L.xr_batch_step_observe_u8(None, 0, acts, buf, 16, 2, None) == _lib.XR_ERR_INVALID
    assert b"xr_batch_step_observe_u8" in L.xr_last_error()
    assert L.xr_batch_observation_u8(None, buf, 16, 0, 1, None) == _lib.XR_ERR_INVALID
    assert L.xr_batch_observation_u8(None, None, 16, 0, 1, None) == _lib.XR_ERR_INVALID
    assert b"xr_batch_observation_u8" in L.xr_last_error()


def test_fixed_spaces_uint8():
    from xroute_env_amd.envs import spaces as sp
    obs, act = sp.fixed_spaces((24, 40, 9), 36, sp=sp, dtype=np.uint8)
    assert obs["grid"].dtype == np.uint8 and obs["grid"].shape == (2 + 7 * 36, 9, 40, 24) and obs["grid"].high == 36.0
    assert {"grid": np.zeros((254, 9, 40, 24), np.uint8), "legal_mask": np.ones(36, np.int8)} in obs
    vec, _ = sp.fixed_spaces((24, 40, 9), 36, batch=8, sp=sp, row=254 * 8640, dtype=np.uint8)
    assert vec["grid"].dtype == np.uint8 and vec["grid"].shape == (8, 254 * 8640)
    assert sp.fixed_spaces((24, 40, 9), 36, sp=sp)[0]["grid"].dtype == np.float32      # the default keeps today's spaces
