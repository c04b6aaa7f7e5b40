"""Peek (xr_batch_peek) without a GPU: the entry point is exported, bound with its argument types and declared in the header with
XR_PEEK_MAX; the header section states the contract; RegionBatch.peek / XRouteVectorEnv.peek check their arguments before the library;
envs.peek's index work (successor_prefix's bit unpacking, the net-indexed tables, the first-maximum pick, the prior) on CPU tensors;
and the validators of the host C++ run under ASan + UBSan as a program of their own (tests/hostsan_peek/peek_args.cpp)."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

from xroute_env_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSAN = os.path.join(ROOT, "tests", "hostsan_peek")


def test_peek_symbol_bound_and_declared():
    L = _lib.lib()
    assert "xr_batch_peek" in _lib.SYMBOLS and hasattr(L, "xr_batch_peek")
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert list(L.xr_batch_peek.argtypes) == [vp, i32, i32, vp, i32, i32, vp, i64, i32, vp, vp, vp, vp, i32, vp]
    assert L.xr_batch_peek.restype is C.c_int32
    hdr = open(os.path.join(ROOT, "include", "xroute_hip.h")).read()
    flat = " ".join(hdr.split())
    assert ("int32_t xr_batch_peek(xr_batch* b, int32_t group, int32_t n_lines, const int32_t* prefix_dev, int32_t prefix_stride, int32_t max_plies, "
            "uint8_t* rows_out_dev, int64_t row_bytes, int32_t region_base, int32_t* out_dev, double* return_out_dev, uint64_t* hash_out_dev, "
            "int32_t* order_out_dev, int32_t k_cap, void* stream);") in flat
    assert "#define XR_ABI_VERSION 9" in hdr and L.xr_abi_version() == 9 and _lib.ABI_VERSION == 9          # an addition: the ABI version stays
    assert _lib.XR_PEEK_MAX == 4096 == _lib.XR_ROLLOUT_MAX
    assert any(l.split()[:3] == ["#define", "XR_PEEK_MAX", "4096"] for l in hdr.splitlines())
    # the section stands after the rollouts and before branch
    assert hdr.index("---- rollouts") < hdr.index("---- peek") < hdr.index("---- branch")


def test_header_section_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "xroute_hip.h")).read()
    sec = " ".join(hdr[hdr.index("---- peek"):hdr.index("---- branch")].split())
    for phrase in ("never synchronises", "one persistent launch", "NO TRACE", "XR_ENV_BAD_ACTION", "costs no ply", "auto-reset", "stream_per_region",
                   "force_scratch_field", "first call", "shadow slots", "rollout's claim counters", "two alternating banks", "ordered by the caller",
                   "XR_ROLLOUT_STOP", "bit for bit", "byte-identical", "xr_batch_pack_state", "16 + 8 * (legal_words + occ_words)", "are not written",
                   "written exactly once", "8-byte aligned", "row_bytes % 8", "xr_batch_state_row_bytes", "31 bits", "XR_PEEK_MAX",
                   "prefix_stride < 1", "negative max_plies", "k_cap < k_max", "the batch is untouched", "DIFFERENT groups"):
        assert phrase in sec, phrase


def test_peek_null_arguments_without_gpu():
    L = _lib.lib()
    out = (C.c_int32 * 16)()
    rows = (C.c_uint64 * 16)()
    for b_rows, b_out in ((None, None), (rows, None), (None, out), (rows, out)):          # (the batch is null in every one)
        assert L.xr_batch_peek(None, -1, 1, None, 0, 0, b_rows, 64, 0, b_out, None, None, None, 0, None) == _lib.XR_ERR_INVALID
        msg = L.xr_last_error()
        assert b"xr_batch_peek" in msg and b"null" in msg


def test_product_library_links_the_peek_kernel():
    """The line launcher (xr_launch_line, kind XR_LINE_PEEK) is weak in csrc/xr_device.h (so that the host-only sanitizer build links): the
    product library must define it."""
    assert hasattr(_lib.lib(), "xr_launch_line")
    dev = open(os.path.join(ROOT, "xroute_env_amd", "csrc", "xr_device.h")).read()
    decl = dev[dev.index("hipError_t xr_launch_line("):]
    assert "__attribute__((weak))" in decl[:decl.index(";")]
    assert "XR_LINE_PEEK" in dev[dev.index("enum XrLineKind"):dev.index("struct XrLineLaunch")]


def _fake_batch():
    import torch
    from xroute_env_amd.batch import RegionBatch
    rb = RegionBatch.__new__(RegionBatch)
    rb.n_envs, rb.device, rb.legal_words, rb.k_max, rb.n_max = 10, torch.device("cpu"), 1, 5, 200          # state_row_bytes = 16 + 8 * (1 + 4) = 56
    rb._group_bounds = [0, 3, 10]
    return rb


def test_region_batch_peek_validates_before_the_library():
    import torch
    rb = _fake_batch()
    L = 2
    bufs = dict(rows_out=torch.zeros((10, L, 56), dtype=torch.uint8), out=torch.zeros((10, L, 8), dtype=torch.int32),
                return_out=torch.zeros((10, L), dtype=torch.float64), hash_out=torch.zeros((10, L), dtype=torch.int64),
                order_out=torch.zeros((10, L, 5), dtype=torch.int32))
    prefix = torch.zeros((10, L, 3), dtype=torch.int32)
    with pytest.raises(ValueError):
        rb.peek(prefix, group=2, **bufs)
    with pytest.raises(ValueError, match="needs n_lines"):
        rb.peek(None, **bufs)
    for bad in (0, -1, _lib.XR_PEEK_MAX + 1):
        with pytest.raises(ValueError, match="n_lines"):
            rb.peek(None, n_lines=bad, **bufs)
    with pytest.raises(ValueError, match="n_lines"):
        rb.peek(torch.zeros((10, 0, 3), dtype=torch.int32), **bufs)
    with pytest.raises(ValueError, match="max_plies"):
        rb.peek(prefix, max_plies=-1, **bufs)
    for bad in (prefix.to(torch.int64), torch.zeros((10, 3, 3), dtype=torch.int32)[:, :2], torch.zeros((10, L), dtype=torch.int32),
                torch.zeros((10, L, 0), dtype=torch.int32), torch.zeros((10, L, 6), dtype=torch.int32)[:, :, ::2],
                torch.zeros((9, L, 3), dtype=torch.int32), prefix.numpy()):
        with pytest.raises(ValueError, match="prefix"):
            rb.peek(bad, **bufs)
    with pytest.raises(ValueError, match="prefix"):
        rb.peek(prefix, n_lines=3, **dict(bufs, rows_out=None, out=None, return_out=None, hash_out=None, order_out=None))          # n_lines disagrees
    for bad in (55, 48, 60, 0, -8):
        with pytest.raises(ValueError, match="row_bytes"):
            rb.peek(prefix, row_bytes=bad, **bufs)
    with pytest.raises(ValueError, match="rows_out"):
        rb.peek(prefix, row_bytes=64, **bufs)                                  # (the buffer's rows are 56 bytes)
    with pytest.raises(ValueError, match="rows_out"):
        rb.peek(prefix, **dict(bufs, rows_out=bufs["rows_out"].to(torch.int8)))
    with pytest.raises(ValueError, match="rows_out"):
        rb.peek(prefix, **dict(bufs, rows_out=torch.zeros((10, L, 112), dtype=torch.uint8)[:, :, ::2]))
    with pytest.raises(ValueError, match="rows_out"):
        rb.peek(prefix[:7].contiguous(), group=1, **bufs)                      # (the group has 7 rows)
    with pytest.raises(ValueError, match="out must"):
        rb.peek(prefix, **dict(bufs, out=bufs["out"].to(torch.int64)))
    with pytest.raises(ValueError, match="return_out"):
        rb.peek(prefix, **dict(bufs, return_out=bufs["return_out"].to(torch.float32)))
    with pytest.raises(ValueError, match="hash_out"):
        rb.peek(prefix, **dict(bufs, hash_out=torch.zeros((10, 3), dtype=torch.int64)))
    with pytest.raises(ValueError, match="order_out"):
        rb.peek(prefix, **dict(bufs, order_out=torch.zeros((10, L, 4), dtype=torch.int32)))
    odd = torch.zeros(10 * L * 56 + 8, dtype=torch.uint8)
    off = next(o for o in range(1, 8) if (odd.data_ptr() + o) % 8)
    with pytest.raises(ValueError, match="8-byte aligned"):
        rb.peek(prefix, **dict(bufs, rows_out=odd[off:off + 10 * L * 56].view(10, L, 56)))


def test_vector_env_peek_has_the_batch_signature_and_refuses_an_unknown_group():
    from xroute_env_amd.batch import RegionBatch
    from xroute_env_amd.envs.vector_env import XRouteVectorEnv
    want = ["prefix", "n_lines", "max_plies", "region_base", "row_bytes", "group"]
    assert list(inspect.signature(XRouteVectorEnv.peek).parameters)[1:] == want
    assert list(inspect.signature(RegionBatch.peek).parameters)[1:] == want + ["stream", "rows_out", "out", "return_out", "hash_out", "order_out"]
    env = XRouteVectorEnv.__new__(XRouteVectorEnv)
    env.batch = _fake_batch()
    env.group_streams, env.n_groups = [None, None], 2
    with pytest.raises(ValueError, match="group"):
        env.peek(None, n_lines=1, group=5)
    env.n_groups = 0
    with pytest.raises(RuntimeError, match="groups"):
        env.peek(None, n_lines=1, group=0)


def test_successor_prefix_bit_unpacking_on_cpu_tensors():
    import torch
    from xroute_env_amd.envs.peek import prefix_from_legal
    rng = np.random.default_rng(11)
    for words, k in ((1, 5), (1, 64), (2, 70), (2, 128), (3, 129), (1, 1)):
        legal = rng.integers(0, 2 ** 63, size=(9, words), dtype=np.int64)
        legal[0] = 0
        legal[1] = -1                                                          # every bit, the sign bit included
        legal[2, 0] = np.int64(-2 ** 63)                                       # only net 64
        got = prefix_from_legal(torch.from_numpy(legal), k)
        assert got.dtype == torch.int32 and tuple(got.shape) == (9, k, 1) and got.is_contiguous()
        bits = ((legal.view(np.uint64)[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(9, -1)[:, :k]
        want = np.zeros((9, k), np.int32)
        for r in range(9):
            nets = np.flatnonzero(bits[r]) + 1
            want[r, :nets.size] = nets
        assert np.array_equal(got[:, :, 0].numpy(), want), (words, k)
        assert np.array_equal(prefix_from_legal(torch.from_numpy(legal.view(np.uint64)), k).numpy(), got.numpy())


def test_pick_best_ties_to_the_lowest_net_and_zero_without_a_candidate():
    import torch
    from xroute_env_amd.envs.peek import _by_net, pick_best
    ninf = float("-inf")
    s = torch.tensor([[ninf, -1.0, -1.0, -3.0], [ninf, ninf, ninf, ninf], [-2.0, ninf, -2.0, -5.0], [-9.0, -8.0, ninf, -7.5], [float("nan"), ninf, ninf, ninf]],
                     dtype=torch.float64)
    act = pick_best(s)
    assert act.dtype == torch.int32 and act.tolist() == [2, 0, 1, 4, 0]
    nets = torch.tensor([[2, 4, 0, 0], [0, 0, 0, 0], [1, 2, 3, 4]], dtype=torch.int32)
    x = torch.tensor([[0.5, 0.25, 9.0, 9.0], [9.0, 9.0, 9.0, 9.0], [1.0, 2.0, 3.0, 4.0]])
    assert _by_net(x, nets, ninf).tolist() == [[ninf, 0.5, ninf, 0.25], [ninf] * 4, [1.0, 2.0, 3.0, 4.0]]


def test_value_prior_is_a_softmax_over_the_candidates_and_its_weights_follow_it():
    import torch
    from xroute_env_amd.envs.peek import value_prior
    from xroute_env_amd.envs.weighted import WEIGHT_ONE
    ninf = float("-inf")
    values = torch.tensor([[0.5, ninf, -0.5], [ninf, ninf, ninf], [1.0, 1.0, 1.0]], dtype=torch.float32)
    rewards = torch.tensor([[-10.0, ninf, -13.0], [ninf, ninf, ninf], [-4.0, -4.0, -4.0]], dtype=torch.float64)
    prior, w = value_prior(values, rewards, 0.5)
    assert prior.dtype == torch.float32 and w.dtype == torch.int32 and prior.is_contiguous() and w.is_contiguous()
    # row 0: scores -9.5 and -13.5, spread 4 -> z = 0, -1 -> softmax at 0.5: 1 : e^-2
    e = np.exp(-2.0)
    assert np.allclose(prior[0].numpy(), [1 / (1 + e), 0.0, e / (1 + e)], rtol=1e-6) and prior[0, 1] == 0
    assert w[0].tolist() == [WEIGHT_ONE, 0, int(round(e * WEIGHT_ONE))]
    assert prior[1].tolist() == [0.0, 0.0, 0.0] and w[1].tolist() == [0, 0, 0]
    assert np.allclose(prior[2].numpy(), 1 / 3) and w[2].tolist() == [WEIGHT_ONE] * 3
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            value_prior(values, rewards, bad)


def test_peek_host_code_under_asan_ubsan_as_a_program_of_its_own():
    r = subprocess.run(["make", "-C", HOSTSAN, "peek_args"], capture_output=True, text=True)
    assert r.returncode == 0, "build of the peek argument program failed: " + r.stderr[-1500:]
    assert "warning" not in r.stderr, r.stderr[-1500:]
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([os.path.join(HOSTSAN, "peek_args")], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("PEEK_ARGS_OK "), (out.stdout[-1500:], out.stderr[-3000:])
    assert out.stderr == "", out.stderr[-3000:]
