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


def test_obs_writer_shape_table_reaches_every_class():
    """The shape table of tests/test_gpu_obs_writers.py (tests/helpers.py) still reaches every class the observation writers branch
    on — conditions on the table and the generator, not measurements: an edit that drops a class fails here, without a GPU."""
    from oracle import xr_oracle as orc
    from tests import helpers as H
    regions = {name: H.obs_set_regions(name) for name in H.OBS_SETS}
    for name, rs in regions.items():
        assert rs and all(r.n_nets >= 1 for r in rs), name                      # every generated region has at least one net
        for r in rs:
            orc.OracleEnv(r)                                                     # and the oracle takes it
    ns = sorted({r.n_nodes for rs in regions.values() for r in rs})
    assert {d[0] * d[1] * d[2] for ds in H.OBS_SHAPE_SETS.values() for d in ds} <= set(ns)
    # where a unit starts in its 16-byte slot: all sixteen residues, odd ones included
    assert {((2 + 7 * rank) * n) % 16 for n in ns for rank in range(9)} == set(range(16))
    assert {n % 2 for n in ns if n >= 128} == {0, 1}
    assert any(2 * n < 16 for n in ns) and any(7 * n < 128 for n in ns)         # planes 0..1 without a whole slot, a unit without a whole line
    assert any(n % 4 == 0 and n % 16 != 0 for n in ns)                          # fp32 aligned, uint8 not
    assert any(n % 16 == 0 for n in ns) and any(n % 4 for n in ns)
    assert any(n > 1024 and n % 2 for n in ns)
    # the mixed batch: aligned regions beside others, so that the aligned ones take the stream writers too
    mixed = [r.n_nodes for r in regions["mixed"]]
    assert any(n % 16 == 0 for n in mixed) and any(n % 4 for n in mixed) and any(n % 4 == 0 and n % 16 for n in mixed + ns)
    assert len(set(mixed)) > 4
    # ids of 128 and more, three legal words and more
    many = regions["many_nets"]
    assert all(128 < r.n_nets <= 255 for r in many) and all((r.n_nets + 63) // 64 >= 3 for r in many)
    # exactly 255 nets: the uint8 limit itself, once with every net legal after a reset and once only declared (the region of the
    # 256-net refusal test); the oracle builds the observation, ids up to 255
    r255, declared = regions["exactly_255"][:2]
    assert r255.n_nets == 255 and declared.n_nets == 255 and max(r.n_nets for r in regions["exactly_255"]) == 255
    ids = np.arange(1, 256, dtype=np.int32)
    assert np.array_equal(orc.OracleEnv(r255).legal(), ids) and 0 < orc.OracleEnv(declared).nlegal() < 255
    for r in (r255, declared):
        obs = orc.build_observation(r.dims, r.nodes, ids)
        planes = obs.reshape(obs.shape[0], r.n_nodes)
        assert obs.shape[0] == 2 + 7 * 255 and np.array_equal(planes[1, :255], ids.astype(np.float32))
        assert planes[2:9].any() and planes[2 + 7 * 254:].any() == (r is r255)   # a net without access points: seven planes of zeros
        assert (obs == np.round(obs)).all() and obs.min() >= 0 and obs.max() == 255
