"""Weighted net sampling (XR-Pick v1) without a GPU: the three entry points are exported, bound with their argument types, declared in
the header and listed in the generated INTEGRATION stub; null arguments are refused without a device; the spec's twin
(tests/weighted_twin.py) has the properties the spec promises; envs.weighted.quantise / weights_from_scores keep range, zeros, maximum
and order; RegionBatch checks its arguments before the library; the product library links the two new launchers; and the validators of
the host C++ run under ASan + UBSan as a program of their own (tests/hostsan_weighted/weighted_args.cpp)."""
import ctypes as C
import os
import random
import subprocess

import pytest

from tests import weighted_twin as wt
from xroute_env_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSAN = os.path.join(ROOT, "tests", "hostsan_weighted")
NAMES = ("xr_batch_weighted_actions", "xr_batch_rollout_weighted", "xr_batch_tree_search_weighted")


def test_weighted_symbols_bound_declared_and_in_the_stub():
    L = _lib.lib()
    vp, i32, u64, f64 = C.c_void_p, C.c_int32, C.c_uint64, C.c_double
    want = {"xr_batch_weighted_actions": [vp, i32, vp, i32, vp, u64, vp],
            "xr_batch_rollout_weighted": list(L.xr_batch_rollout.argtypes[:-1]) + [vp, i32, vp],
            "xr_batch_tree_search_weighted": list(L.xr_batch_tree_search.argtypes[:-1]) + [vp, vp]}
    assert want["xr_batch_rollout_weighted"] == [vp, i32, i32, i32, u64, vp, i32, i32, vp, vp, vp, vp, i32, vp, i32, vp]
    assert want["xr_batch_tree_search_weighted"] == [vp, i32, i32, i32, u64, vp, i32, f64, f64, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    hdr = open(os.path.join(ROOT, "include", "xroute_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        assert list(getattr(L, name).argtypes) == want[name], name
        assert getattr(L, name).restype is C.c_int32, name
        assert f"int32_t {name}(xr_batch* b, int32_t group," in hdr, name
        assert f"#   {name}(" in doc, name
    assert "#define XR_ABI_VERSION 9" in hdr and L.xr_abi_version() == 9          # an addition: the ABI version stays
    for name, value, text in (("XR_ROLLOUT_WEIGHTED", 2, "2"), ("XR_WEIGHT_MAX", 1 << 24, "(1 << 24)")):
        assert getattr(_lib, name) == value
        assert any(l.startswith(f"#define {name} ") and l.split(None, 2)[2].startswith(text) for l in hdr.splitlines()), name
    assert wt.WEIGHT_MAX == _lib.XR_WEIGHT_MAX
    sec = hdr[hdr.index("---- weighted net sampling"):hdr.index("---- XR-Maze v2: global-route guides")]
    for phrase in ("XR-Pick v1", "0x100000001B3", "r % L", "t = r % S", "min(w, XR_WEIGHT_MAX)", "never validated on the host", "only enqueues",
                   "xr_batch_rollout itself keeps refusing policy 2", "NULL sim_weights_dev", "weights_k_cap < k_max", "Cuts:"):
        assert phrase in sec, phrase


def test_weighted_null_arguments_without_gpu():
    L = _lib.lib()
    buf = (C.c_int32 * 16)()
    for args in ((None, -1, buf, 4, buf, 0, None), (None, -1, None, 4, None, 0, None)):
        assert L.xr_batch_weighted_actions(*args) == _lib.XR_ERR_INVALID
        assert b"xr_batch_weighted_actions" in L.xr_last_error() and b"null" in L.xr_last_error()
    assert L.xr_batch_rollout_weighted(None, -1, 1, 2, 0, None, 0, 0, buf, None, None, None, 0, buf, 4, None) == _lib.XR_ERR_INVALID
    assert b"xr_batch_rollout_weighted" in L.xr_last_error() and b"null" in L.xr_last_error()
    assert L.xr_batch_tree_search_weighted(None, -1, 1, 1, 0, None, 8, 1.25, 19652.0, buf, buf, 4, buf, None, None, None, None, buf,
                                           None) == _lib.XR_ERR_INVALID
    assert b"xr_batch_tree_search_weighted" in L.xr_last_error() and b"null" in L.xr_last_error()
    # the old entry points name themselves as before
    assert L.xr_batch_rollout(None, -1, 1, 1, 0, None, 0, 0, None, None, None, None, 0, None) == _lib.XR_ERR_INVALID
    assert b"xr_batch_rollout:" in L.xr_last_error()


def test_product_library_links_the_weighted_launchers():
    """The launchers are weak in csrc/xr_device.h (so that the host-only sanitizer build links): the product library must define them."""
    L = _lib.lib()
    assert hasattr(L, "xr_launch_weighted_actions") and hasattr(L, "xr_launch_line")          # (the rollout under weights: kind XR_LINE_WEIGHTED)
    dev = open(os.path.join(ROOT, "xroute_env_amd", "csrc", "xr_device.h")).read()
    assert "XR_LINE_WEIGHTED" in dev[dev.index("enum XrLineKind"):dev.index("struct XrLineLaunch")]


# ---- the twin's properties -------------------------------------------------------------------------------------------------------------
def _cases(n, seed):
    rng = random.Random(seed)
    for _ in range(n):
        k = rng.choice((1, 2, 5, 63, 64, 65, 70, 130, 260))
        legal = [net for net in range(1, k + 1) if rng.random() < rng.choice((0.1, 0.5, 1.0))]
        yield rng, k, legal, rng.getrandbits(64)


def test_twin_unit_and_all_zero_weights_are_the_uniform_pick():
    seen = 0
    for rng, k, legal, r in _cases(3000, 1):
        want = sorted(legal)[r % len(legal)] if legal else 0
        assert wt.pick_from_r(legal, [1] * k, r) == want
        assert wt.pick_from_r(legal, [0] * k, r) == want
        assert wt.pick_from_r(legal, [rng.randint(-2 ** 31, 0) for _ in range(k)], r) == want           # negatives count as 0
        if legal:          # everything above the clamp counts 2^24: net number (r % (L * 2^24)) // 2^24
            M = wt.WEIGHT_MAX
            assert wt.pick_from_r(legal, [rng.randint(M, 2 ** 31 - 1) for _ in range(k)], r) == sorted(legal)[r % (len(legal) * M) // M]
        seen += bool(legal)
    assert seen > 2000


def test_twin_a_zero_weight_net_is_never_picked_beside_a_positive_one_and_a_single_positive_weight_always_wins():
    mixed = 0
    for rng, k, legal, r in _cases(3000, 2):
        if not legal:
            continue
        w = [rng.choice((0, 0, -7, rng.randint(1, 1 << 25))) for _ in range(k)]
        p = wt.pick_from_r(legal, w, r)
        assert p in legal
        if any(w[n - 1] > 0 for n in legal):
            assert w[p - 1] > 0, (legal, w, r, p)
            mixed += any(w[n - 1] <= 0 for n in legal)
        one = rng.choice(legal)
        solo = [rng.randint(-5, 0) for _ in range(k)]
        solo[one - 1] = rng.choice((1, 17, 1 << 24, 2 ** 31 - 1))
        assert wt.pick_from_r(legal, solo, r) == one
    assert mixed > 500


def test_twin_clamps_at_2_24_and_follows_the_running_sum():
    assert [wt.effective(v) for v in (-2 ** 31, -1, 0, 1, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, 2 ** 31 - 1)] == \
        [0, 0, 0, 1, (1 << 24) - 1, 1 << 24, 1 << 24, 1 << 24]
    legal, M = [2, 3, 7, 66], 1 << 24
    w = [0] * 70
    w[1], w[2], w[6], w[65] = 3, 2 ** 31 - 1, 1, 5                        # q = 3, 2^24, 1, 5; a large weight on the illegal net 5 is never read
    w[4] = 2 ** 31 - 1
    S = 3 + M + 1 + 5
    for t, want in ((0, 2), (2, 2), (3, 3), (3 + M - 1, 3), (3 + M, 7), (3 + M + 1, 66), (S - 1, 66)):
        for lap in (0, 1, 12345):
            assert wt.pick_from_r(legal, w, t + lap * S) == want, (t, lap)
    assert wt.pick_from_r(legal, w[:10], 3 + M + 1) == 2                  # a weight row that ends before net 66: the net counts 0 (t = 0 of S = 3 + M + 1)
    assert wt.pick_from_r([], w, 99) == 0
    # the hash: the documented composition, 64-bit wrap included
    assert wt.splitmix64(0) == 0xE220A8397B1DCDAF
    assert wt.pick_hash(5, 3, 9) == wt.splitmix64(5 ^ wt.splitmix64(3 * 0x100000001B3 + 9))
    assert wt.pick_hash(2 ** 64 + 5, 3, 9) == wt.pick_hash(5, 3, 9)
    assert wt.legal_nets([0b101, 1 << 63, 0, 1]) == [1, 3, 128, 193]


def test_twin_frequencies_follow_the_weights():
    """Not a statistical test of the hash: over ALL residues t in [0, S) every net owns exactly q(n) of them."""
    legal, w = [1, 4, 5, 9], [5, 0, 0, 1, 0, 0, 0, 0, 10]
    counts = {n: 0 for n in legal}
    for t in range(16):
        counts[wt.pick_from_r(legal, w, t + 16 * 977)] += 1
    assert counts == {1: 5, 4: 1, 5: 0, 9: 10}


# ---- quantise / weights_from_scores --------------------------------------------------------------------------------------------------
def test_quantise_range_zeros_maximum_and_order():
    import torch
    from xroute_env_amd.envs.weighted import WEIGHT_ONE, quantise, weights_from_scores
    assert WEIGHT_ONE == 1 << 20
    g = torch.Generator().manual_seed(3)
    p = torch.rand((200, 37), generator=g, dtype=torch.float64) ** 8 * 1e6          # many tiny entries beside large ones
    p[torch.rand((200, 37), generator=g) < 0.2] = 0.0
    p[0, 0], p[1, 1], p[2, 2], p[3, 3] = float("nan"), float("inf"), -float("inf"), -3.0
    p[4] = 0.0                                                                     # a row without a positive entry
    q = quantise(p)
    assert q.dtype == torch.int32 and q.shape == p.shape
    ok = torch.isfinite(p) & (p > 0)
    assert int(q.min()) >= 0 and int(q.max()) == WEIGHT_ONE
    assert torch.equal(q == 0, ~ok)                                                # a zero only for a non-finite or non-positive input
    clean = torch.where(ok, p, torch.zeros_like(p))
    has = ok.any(dim=1)
    assert torch.equal(q.max(dim=1).values[has], torch.full((int(has.sum()),), WEIGHT_ONE, dtype=torch.int32))
    assert (q.gather(1, clean.argmax(dim=1, keepdim=True)).squeeze(1)[has] == WEIGHT_ONE).all()      # the row maximum maps to 2^20
    a, b = clean.unsqueeze(2), clean.unsqueeze(1)
    qa, qb = q.unsqueeze(2), q.unsqueeze(1)
    assert not ((a < b) & (qa > qb)).any()                                         # the order is preserved (ties may appear, inversions not)
    want = torch.round(clean[7] / clean[7].max() * 2 ** 20).clamp_min(1).to(torch.int32)
    assert torch.equal(q[7], torch.where(ok[7], want, torch.zeros_like(want)))     # the formula itself
    assert quantise(p.to(torch.float32)).dtype == torch.int32
    # scores: a softmax over the finite entries
    s = torch.randn((50, 21), generator=g, dtype=torch.float64) * 30
    s[torch.rand((50, 21), generator=g) < 0.3] = -float("inf")
    s[0, 0], s[1, 1] = float("nan"), float("inf")
    s[2] = -float("inf")
    s[3, :2] = torch.tensor([0.0, -5000.0])                                        # exp underflows: the net still keeps a chance
    for temp in (0.5, 1.0, 40.0):
        w = weights_from_scores(s, temp)
        fin = torch.isfinite(s)
        assert w.dtype == torch.int32 and int(w.min()) >= 0 and int(w.max()) == WEIGHT_ONE
        assert torch.equal(w == 0, ~fin)
        low = torch.where(fin, s, torch.full_like(s, -float("inf")))
        rows = fin.any(dim=1)
        assert (w.gather(1, low.argmax(dim=1, keepdim=True)).squeeze(1)[rows] == WEIGHT_ONE).all()
        assert not ((low.unsqueeze(2) < low.unsqueeze(1)) & (w.unsqueeze(2) > w.unsqueeze(1)) & fin.unsqueeze(2) & fin.unsqueeze(1)).any()
        assert int(w[3, 1]) == 1 if temp < 40 else int(w[3, 1]) >= 1
    e = torch.exp((s[5] - s[5][torch.isfinite(s[5])].max()) / 2.0)
    want = torch.where(torch.isfinite(s[5]), torch.round(e * 2 ** 20).clamp_min(1), torch.zeros_like(e)).to(torch.int32)
    assert torch.equal(weights_from_scores(s, 2.0)[5], want)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            weights_from_scores(s, bad)


def test_region_batch_weighted_calls_validate_before_the_library():
    import torch
    from xroute_env_amd.batch import RegionBatch
    from xroute_env_amd.envs.weighted import cem_search
    rb = RegionBatch.__new__(RegionBatch)          # no handle, no library: anything that got past the checks would fail on `_h`
    rb.n_envs, rb.device, rb.legal_words, rb.k_max = 10, torch.device("cpu"), 1, 5
    rb._group_bounds = [0, 3, 10]
    good = torch.ones((10, 5), dtype=torch.int32)
    bad_weights = (good.to(torch.int64), good.to(torch.float32), torch.ones((10, 4), dtype=torch.int32), torch.ones((9, 5), dtype=torch.int32),
                   torch.ones((10, 5, 1), dtype=torch.int32), torch.ones((10, 10), dtype=torch.int32)[:, ::2], torch.ones((10, 5), dtype=torch.int32,
                                                                                                                       device="meta"),
                   [[1] * 5] * 10, None)
    bufs = dict(out=torch.zeros((10, 2, 8), dtype=torch.int32), return_out=torch.zeros((10, 2), dtype=torch.float64),
                hash_out=torch.zeros((10, 2), dtype=torch.int64), order_out=torch.zeros((10, 2, 5), dtype=torch.int32))
    for w in bad_weights:
        with pytest.raises(ValueError, match="weights"):
            rb.weighted_actions(w, 7)
        with pytest.raises(ValueError, match="weights"):
            rb.rollout(2, policy="weighted", weights=w, **bufs)
        if w is not None:
            with pytest.raises(ValueError, match="sim_weights"):
                rb.tree_search(2, 2, sim_weights=w)
    with pytest.raises(ValueError, match="weights"):
        rb.weighted_actions(good, 7, group=1)                                  # (the group has 7 rows)
    with pytest.raises(ValueError):
        rb.weighted_actions(good, 7, group=2)
    for out in (torch.zeros(10, dtype=torch.int64), torch.zeros(9, dtype=torch.int32), torch.zeros((10, 1), dtype=torch.int32),
                torch.zeros(20, dtype=torch.int32)[::2]):
        with pytest.raises(ValueError, match="out must"):
            rb.weighted_actions(good, 7, out=out)
    # weights belong to the weighted policy, and to no other
    for pol in ("random", "stop", 0, 1):
        with pytest.raises(ValueError, match="weights"):
            rb.rollout(2, policy=pol, weights=good, **bufs)
    for pol in ("weighted", 2):
        with pytest.raises(ValueError, match="weights"):
            rb.rollout(2, policy=pol, **bufs)
    with pytest.raises(ValueError, match="policy"):
        rb.rollout(2, policy=3, weights=good, **bufs)
    for kw in (dict(n_iters=0, n_rollouts=4, n_elite=2), dict(n_iters=2, n_rollouts=0, n_elite=1), dict(n_iters=2, n_rollouts=4, n_elite=5),
               dict(n_iters=2, n_rollouts=4, n_elite=0), dict(n_iters=2, n_rollouts=4, n_elite=2, smoothing=0.0),
               dict(n_iters=2, n_rollouts=4, n_elite=2, tau=0.0)):
        with pytest.raises(ValueError):
            cem_search(rb, **kw)


def test_weighted_host_code_under_asan_ubsan_as_a_program_of_its_own():
    r = subprocess.run(["make", "-C", HOSTSAN, "weighted_args"], capture_output=True, text=True)
    assert r.returncode == 0, "build of the weighted argument program failed: " + r.stderr[-1500:]
    assert "warning" not in r.stderr, r.stderr[-1500:]
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([os.path.join(HOSTSAN, "weighted_args")], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("WEIGHTED_ARGS_OK "), (out.stdout[-1500:], out.stderr[-3000:])
    assert out.stderr == "", out.stderr[-3000:]
