"""Kept trees (xr_batch_tree_search_keep, "XR-Tree v1, kept") without a GPU: the entry point is exported, bound, declared in its place and
present in the INTEGRATION stub; null arguments are refused without a device; RegionBatch.tree_search checks `played` before the library;
the spec's twin (tests/tree_keep_twin.py) on hand-made returns; and the validators of the host C++ under ASan + UBSan as a program of
their own (tests/hostsan_tree_keep/tree_keep_args.cpp)."""
import ctypes as C
import os
import subprocess

import pytest

from tests import tree_keep_twin as kt
from tests import tree_twin
from xroute_env_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSAN = os.path.join(ROOT, "tests", "hostsan_tree_keep")
INF = float("inf")
KEPT, FULL = kt.KEPT, tree_twin.POOL_FULL


def test_keep_symbol_bound_declared_and_in_the_stub():
    L = _lib.lib()
    vp, i32, f64 = C.c_void_p, C.c_int32, C.c_double
    assert "xr_batch_tree_search_keep" in _lib.SYMBOLS and hasattr(L, "xr_batch_tree_search_keep")
    assert L.xr_batch_tree_search_keep.restype is i32
    assert list(L.xr_batch_tree_search_keep.argtypes) == [vp, i32, vp, i32, i32, C.c_uint64, vp, i32, f64, f64, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    hdr = open(os.path.join(ROOT, "include", "xroute_hip.h")).read()
    assert "int32_t xr_batch_tree_search_keep(xr_batch* b, int32_t group, const int32_t* played_dev," in hdr
    assert "#define XR_ABI_VERSION 9" in hdr and L.xr_abi_version() == 9          # an addition: the ABI version stays
    assert _lib.XR_TREE_KEPT == 2 == kt.KEPT
    assert any(l.split()[:3] == ["#define", "XR_TREE_KEPT", "2"] for l in hdr.splitlines())
    # the section is in its place, and its title is not a second "---- tree search"
    a, k, m = hdr.index("---- weighted net sampling"), hdr.index("---- kept trees"), hdr.index("---- XR-Maze v2: global-route guides")
    assert a < k < m and hdr.count("---- tree search") == 1 and hdr.index("---- tree search") < a
    sec = hdr[k:m]
    for phrase in ("XR-Tree v1, kept", "Own memory", "80 node_cap", "played_dev", "env_steps == key.env_steps + 1", "breadth-first",
                   "W' = W - (double)N * r", "min' = min - r", "XR_TREE_KEPT", "XR_TREE_MAX_SIMS", "kept_out_dev", "does not carry",
                   "never an", "stream_per_region"):
        assert phrase in sec, phrase
    assert "no tree reuse" in hdr[hdr.index("---- tree search"):a]                 # the plain search's documented cut stays
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "xr_batch_tree_search_keep(vp, c_int, vp, c_int, c_int, c_ulong, vp, c_int, c_double, c_double" in doc


def test_product_library_links_the_keep_kernel():
    assert hasattr(_lib.lib(), "xr_launch_tree_keep_begin")


def test_keep_null_arguments_without_gpu():
    L = _lib.lib()
    args = (2, 2, 0, None, 8, 1.25, 19652.0)
    assert L.xr_batch_tree_search_keep(None, -1, None, *args, None, None, 4, None, None, None, None, None, None, None, None) == _lib.XR_ERR_INVALID
    msg = L.xr_last_error()
    assert b"xr_batch_tree_search_keep" in msg and b"null" in msg
    v, val, info = (C.c_int32 * 16)(), (C.c_double * 16)(), (C.c_int32 * 16)()
    assert L.xr_batch_tree_search_keep(None, -1, None, *args, v, val, 4, info, None, None, None, None, None, None, None) == _lib.XR_ERR_INVALID
    assert b"xr_batch_tree_search_keep" in L.xr_last_error()


def test_region_batch_refuses_bad_played_before_the_library():
    import torch
    from xroute_env_amd.batch import RegionBatch
    rb = RegionBatch.__new__(RegionBatch)          # no handle, no library: whatever gets past the checks fails on the missing attributes
    rb.n_envs, rb.device, rb.legal_words, rb.k_max = 10, torch.device("cpu"), 1, 5
    rb._group_bounds = [0, 3, 10]
    for bad in (torch.zeros(10, dtype=torch.int64), torch.zeros(9, dtype=torch.int32), torch.zeros((10, 1), dtype=torch.int32),
                torch.zeros(20, dtype=torch.int32)[::2], [0] * 10, torch.zeros(10, dtype=torch.int32, device="meta")):
        with pytest.raises(ValueError, match="played"):
            rb.tree_search(2, 2, keep=True, played=bad)
    with pytest.raises(ValueError, match="played"):
        rb.tree_search(2, 2, keep=True, played=torch.zeros(10, dtype=torch.int32), group=1)          # (the group has 7 rows)
    with pytest.raises(ValueError, match="played"):
        rb.tree_search(2, 2, played=torch.zeros(10, dtype=torch.int32))                               # played without keep
    with pytest.raises(ValueError, match="n_waves"):
        rb.tree_search(0, 2, keep=True)                                                               # the shared checks still come first
    with pytest.raises(Exception) as ei:                                                              # a good one gets past the checks
        rb.tree_search(2, 2, keep=True, played=torch.zeros(10, dtype=torch.int32))
    assert not isinstance(ei.value, ValueError), ei.value


# ---- the twin on hand-made returns -------------------------------------------------------------------------------------------------
R = -0.3          # the reward of the played step: not a dyadic number, so W - N * r rounds
LONG = None


def _E():
    global LONG
    if LONG is None:
        LONG = _lib.tree_exploration_table(1.25, 19652.0, kt.MAX_SIMS)
    return LONG


def _value(p):
    """G of a simulation whose path is p: a different, non-dyadic number per path."""
    g = -1.0
    for d, n in enumerate(p):
        g = g - 0.1 * n / (d + 1.0)
    return g


def _evaluate(legal, value=_value):
    def evaluate(w, paths):
        return ([[value(tuple(p)) for p in row] for row in paths],
                [[list(p) + [n for n in sorted(legal) if n not in p] for p in row] for row in paths])
    return evaluate


def _first_call(legal, n_waves=6, n_par=2, node_cap=200, prior=None, value=_value):
    """A pool of one row after a fresh kept call from State(3, 7, 2, legal)."""
    pool = kt.KeptPool()
    st = kt.State(3, 7, 2, legal)
    res, _, _, trees = pool.search([st], None, n_waves, n_par, node_cap, _E(), _evaluate(legal, value), max(legal),
                                   None if prior is None else [prior])
    return pool, st, res[0], trees[0]


def _after(st, a, reward=R, **kw):
    d = dict(env_steps=st.env_steps + 1, region=st.region, replay=st.replay, legal=[n for n in st.legal if n != a], reward=reward)
    d.update(kw)
    return kt.State(**d)


def _most_visited(tree):
    root = tree.nodes[0]
    return max(range(root.first, root.first + root.count), key=lambda i: (tree.nodes[i].N, -i))


def _same_tree(a, b):
    fields = ("N", "V", "W", "P", "net", "first", "count")
    return len(a.nodes) == len(b.nodes) and all(getattr(x, f) == getattr(y, f) for x, y in zip(a.nodes, b.nodes) for f in fields) and \
        (a.mn, a.mx, a.best, a.flags, a.max_depth, a.legal) == (b.mn, b.mx, b.best, b.flags, b.max_depth, b.legal)


def test_the_fresh_kept_call_is_the_plain_twin():
    legal = [1, 2, 3, 5]
    _, _, res, tree = _first_call(legal)
    plain, _, _, trees = tree_twin.search([legal], 6, 2, 200, _E(), _evaluate(legal), 5)
    assert _same_tree(tree, trees[0]) and res["kept"] == [0, 0]
    assert {k: v for k, v in res.items() if k != "kept"} == plain[0] and res["info"][3] == 0


def test_a_reroot_carries_the_grandchildren_shifted_to_the_bit_and_numbers_breadth_first():
    legal = [1, 2, 3, 5]
    pool, st, _, old = _first_call(legal, n_waves=12)
    ci = _most_visited(old)
    a = old.nodes[ci].net
    assert old.nodes[ci].first >= 0 and old.max_depth >= 3
    tree, kept = pool.rows[0].begin(_after(st, a), a, 0, 200, _E())          # no further simulation
    assert kept == [old.nodes[ci].N, len(tree.nodes)] and kept[0] > 0 and tree.flags == KEPT
    # the new root: the old child; its children: the old grandchildren, N kept, W - N * r as two operations
    root, oc = tree.nodes[0], old.nodes[ci]
    assert (root.net, root.P, root.N, root.count, root.first) == (0, 1.0, oc.N, oc.count, 1)
    assert root.W == oc.W - float(oc.N) * R and root.W != oc.W
    for j in range(oc.count):
        g, n = old.nodes[oc.first + j], tree.nodes[1 + j]
        nr = float(g.N) * R
        assert (n.N, n.P, n.net, n.count, n.V) == (g.N, g.P, g.net, g.count, 0) and n.W == g.W - nr
    assert any(n.N > 0 and n.W != 0.0 for n in tree.nodes[1:1 + oc.count])
    # breadth first: the blocks of the expanded nodes, in index order, tile [1, used) without a gap; nets ascend inside a block
    nxt = 1
    for n in tree.nodes:
        if n.first >= 0:
            assert n.first == nxt and n.count > 0
            nets = [tree.nodes[i].net for i in range(n.first, n.first + n.count)]
            assert nets == sorted(nets)
            nxt += n.count
    assert nxt == len(tree.nodes) and sum(1 for n in tree.nodes if n.first >= 0) >= 3
    # visits are conserved below every kept node: N of an expanded, non-terminal node = its children's sum + the visit that expanded it
    for n in tree.nodes:
        if n.first >= 0:
            assert n.N == 1 + sum(tree.nodes[i].N for i in range(n.first, n.first + n.count))
    # the row state: shifted by r, best and depth restart
    assert (tree.mn, tree.mx) == (old.mn - R, old.mx - R) and tree.best == -INF and tree.max_depth == 0 and tree.sims == 0
    assert tree.legal == [n for n in legal if n != a]
    res = tree.result(5)
    assert res["info"] == [0, len(tree.nodes), 0, KEPT]
    assert [res["visits"][tree.nodes[1 + j].net - 1] for j in range(oc.count)] == [old.nodes[oc.first + j].N for j in range(oc.count)]


def test_a_continued_search_adds_to_the_carried_visits_and_reads_the_long_table():
    legal = [1, 2, 3, 5, 6]
    pool, st, _, old = _first_call(legal, n_waves=10, n_par=3)
    ci = _most_visited(old)
    a, carried = old.nodes[ci].net, old.nodes[ci].N
    st2 = _after(st, a)
    seen = []

    class Spy(list):
        def __getitem__(self, i):
            seen.append(i)
            return list.__getitem__(self, i)
    res, paths, _, trees = pool.search([st2], [a], 2, 2, 200, Spy(_E()), _evaluate(st2.legal), 6)
    assert carried > 4 and max(seen) >= carried + 3 > 2 * 2          # the root's count is above this call's simulations: no clamp there
    assert res[0]["kept"][0] == carried and res[0]["info"][0] == 4 and res[0]["info"][3] == KEPT
    assert sum(res[0]["visits"]) == carried - 1 + 4 and trees[0].nodes[0].N == carried + 4
    assert res[0]["best_return"] == max(_value(tuple(n for n in p if n)) for p in paths[0])          # the best line is this call's


def test_played_zero_keeps_everything():
    legal = [1, 2, 3]
    pool, st, first, old = _first_call(legal, n_waves=2, n_par=2)
    res, _, _, trees = pool.search([st], [0], 2, 2, 200, _E(), _evaluate(legal), 3)
    two, _, _, t2 = tree_twin.search([legal], 4, 2, 200, _E(), _evaluate(legal), 3)
    assert res[0]["kept"] == [4, len(old.nodes)] and res[0]["info"] == [4, two[0]["info"][1], res[0]["info"][2], KEPT]
    assert sum(res[0]["visits"]) == 8 and res[0]["visits"] == two[0]["visits"] and res[0]["value"] == two[0]["value"]
    assert [(n.N, n.W, n.net, n.first) for n in trees[0].nodes] == [(n.N, n.W, n.net, n.first) for n in t2[0].nodes]
    assert (trees[0].mn, trees[0].mx) == (t2[0].mn, t2[0].mx)


def test_every_key_mismatch_rebuilds_and_equals_a_fresh_tree():
    legal = [1, 2, 3, 5]
    for what, played, make, cap in (
            ("wrong net", lambda a: 5 if a != 5 else 3, lambda st, a: _after(st, a), 200),
            ("a net that is not legal", lambda a: 4, lambda st, a: _after(st, a), 200),
            ("two steps", lambda a: a, lambda st, a: _after(_after(st, a), [n for n in legal if n != a][0]), 200),
            ("no step", lambda a: a, lambda st, a: st, 200),
            ("played 0 after a step", lambda a: 0, lambda st, a: _after(st, a), 200),
            ("legal set changed", lambda a: a, lambda st, a: _after(st, a, legal=[n for n in legal if n != a][1:]), 200),
            ("another region", lambda a: a, lambda st, a: _after(st, a, region=8), 200),
            ("another replay", lambda a: a, lambda st, a: _after(st, a, replay=3), 200),
            ("a negative entry", lambda a: -1, lambda st, a: _after(st, a), 200),
            ("root unexpanded: its pool was full", lambda a: a, lambda st, a: _after(st, a), 4)):
        pool, st, _, old = _first_call(legal, node_cap=cap)
        if cap == 4:
            assert old.nodes[0].first < 0 and old.flags == FULL
            a = 1
        else:
            a = old.nodes[_most_visited(old)].net
        st2 = make(st, a)
        tree, kept = pool.rows[0].begin(st2, played(a), 4, cap, _E())
        assert kept == [0, 0] and _same_tree(tree, tree_twin.RowTree(st2.legal, cap, _E())), what
        assert not tree.flags & KEPT, what
    # a net that is legal but no child of the root cannot happen on a consistent tree: a tree whose root block lost it
    pool, st, _, old = _first_call(legal)
    old.nodes[old.nodes[0].first].net = 99
    st2 = _after(st, 1)
    tree, kept = pool.rows[0].begin(st2, 1, 4, 200, _E())
    assert kept == [0, 0] and _same_tree(tree, tree_twin.RowTree(st2.legal, 200, _E())), "net not a child"
    # the visit limit: a child whose N + the call's simulations is above XR_TREE_MAX_SIMS
    pool, st, _, old = _first_call(legal)
    ci = _most_visited(old)
    a = old.nodes[ci].net
    old.nodes[ci].N = kt.MAX_SIMS - 3
    assert pool.rows[0]._mode(_after(st, a), a, 3)[0] == 2 and pool.rows[0]._mode(_after(st, a), a, 4)[0] == 0
    # another shape: the host rebuilds every row
    for shape in (dict(node_cap=201), dict(k_cap=6), dict(lo=1)):
        pool, st, _, old = _first_call(legal)
        kw = dict(dict(node_cap=200, k_cap=5, lo=0), **shape)
        res, _, _, _ = pool.search([st], [0], 1, 1, kw["node_cap"], _E(), _evaluate(legal), kw["k_cap"], lo=kw["lo"])
        assert res[0]["kept"] == [0, 0] and res[0]["info"][3] == 0, shape


def test_an_unexpanded_chosen_child_is_expanded_with_this_calls_prior():
    legal = [1, 2, 3]
    # node_cap 1 + 3 + 2: the root's block and one child's; the last lane of the wave meets a full pool and leaves its child unexpanded
    pool, st, _, old = _first_call(legal, n_waves=1, n_par=2, node_cap=6)
    root = old.nodes[0]
    kids = [old.nodes[i] for i in range(root.first, root.first + root.count)]
    closed = [k for k in kids if k.first < 0 and k.N == 1]
    assert closed and old.flags == FULL
    a = closed[0].net
    st2 = _after(st, a)
    prior = [0.0, 0.0, 0.0]
    rest = st2.legal
    prior[rest[0] - 1], prior[rest[1] - 1] = 1.0, 3.0
    tree, kept = pool.rows[0].begin(st2, a, 2, 6, _E(), prior)
    assert kept == [1, 1] and tree.flags == KEPT and tree.nodes[0].N == 1 and tree.nodes[0].W == closed[0].W - 1.0 * R
    assert [(n.net, n.P, n.N) for n in tree.nodes[1:]] == [(rest[0], 0.25, 0), (rest[1], 0.75, 0)] and tree.nodes[0].first == 1
    # kept nodes keep the P they were given: a continued search under another prior changes new blocks only
    pool, st, _, old = _first_call([1, 2, 3, 5], n_waves=8)
    ci = _most_visited(old)
    a = old.nodes[ci].net
    tree, _ = pool.rows[0].begin(_after(st, a), a, 2, 200, _E(), [9.0, 1.0, 1.0, 0.0, 1.0])
    oc = old.nodes[ci]
    assert [tree.nodes[1 + j].P for j in range(oc.count)] == [old.nodes[oc.first + j].P for j in range(oc.count)] == [1.0 / 3.0] * 3


def test_a_terminal_chosen_child_gives_a_done_row():
    pool, st, _, old = _first_call([4], n_waves=2, n_par=2)
    st2 = _after(st, 4)
    res, paths, returns, trees = pool.search([st2], [4], 2, 2, 200, _E(), lambda w, p: ([[0.0] * 2], [[[], []]]), 4)
    assert trees[0].done and res[0] == dict(visits=[0] * 4, value=[-INF] * 4, info=[0, 0, 0, 0], best_order=[0] * 4, best_return=-INF, kept=[0, 0])
    assert paths[0] == [[0] * 4] * 4 and returns[0] == [0.0] * 4
    # and the next call of that row starts over, whatever it is told
    st3 = kt.State(0, 7, 3, [1, 2])
    for played in (0, 4):
        p2 = kt.KeptPool()
        p2.rows, p2.shape = pool.rows, (1, 0, 200, 4)
        r2, _, _, _ = p2.search([st3], [played], 1, 1, 200, _E(), _evaluate([1, 2]), 4)
        assert r2[0]["kept"] == [0, 0] and r2[0]["info"][3] == 0


def test_a_pool_the_continued_tree_fills_exactly_and_one_more_simulation_overflows():
    legal = [1, 2, 3, 5, 6]

    def run(cap, waves2):
        pool, st, _, old = _first_call(legal, n_waves=3, n_par=1, node_cap=cap)
        a = old.nodes[_most_visited(old)].net
        st2 = _after(st, a)
        res, _, _, _ = pool.search([st2], [a], waves2, 1, cap, _E(), _evaluate(st2.legal), 6)
        return len(old.nodes), res[0]
    used1, roomy = run(1000, 6)
    cap = roomy["info"][1]
    assert roomy["kept"][1] < cap and used1 <= cap and roomy["info"][3] == KEPT
    used1b, exact = run(cap, 6)
    assert used1b == used1 and exact == roomy          # the pool is full to the last node and nobody has noticed
    _, over = run(cap, 7)
    assert over["info"] == [7, cap, over["info"][2], KEPT | FULL] and over["kept"] == roomy["kept"]


def test_keep_host_code_under_asan_ubsan_as_a_program_of_its_own():
    r = subprocess.run(["make", "-C", HOSTSAN, "tree_keep_args"], capture_output=True, text=True)
    assert r.returncode == 0, "build of the kept-tree argument program failed: " + r.stderr[-1500:]
    assert "warning" not in r.stderr, r.stderr[-1500:]
    out = subprocess.run([os.path.join(HOSTSAN, "tree_keep_args")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("TREE_KEEP_ARGS_OK "), (out.stdout[-1500:], out.stderr[-3000:])
    assert out.stderr == "", out.stderr[-3000:]
