"""Evaluated tree search (xr_batch_tree_open / _leaves / _backup, "XR-Tree v2, evaluated") without a GPU: the entry points are exported,
bound, declared in their place and present in the INTEGRATION stub; null arguments and the call order are refused without a device;
RegionBatch.tree_open / tree_leaves / tree_backup check their arguments before the library; the spec's twin (tests/tree_eval_twin.py) on
hand-made values; and the validators of the host C++ under ASan + UBSan as a program of their own
(tests/hostsan_tree_eval/tree_eval_args.cpp)."""
import ctypes as C
import os
import subprocess

import pytest

from tests import tree_eval_twin as et
from tests import tree_twin
from xroute_env_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSAN = os.path.join(ROOT, "tests", "hostsan_tree_eval")
INF = float("inf")
NAN = float("nan")
TERMINAL, FRESH, NONE, FULL = et.TERMINAL, et.FRESH, et.NONE, tree_twin.POOL_FULL
NAMES = ("xr_batch_tree_open", "xr_batch_tree_leaves", "xr_batch_tree_backup")


def test_symbols_bound_typed_declared_and_in_the_stub():
    L = _lib.lib()
    vp, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(L, name) and getattr(L, name).restype is i32, name
    assert list(L.xr_batch_tree_open.argtypes) == [vp, i32, i32, i32, f64, f64, i32, vp, i32, vp]
    assert list(L.xr_batch_tree_leaves.argtypes) == [vp, i32, vp, i64, i32, vp, vp, vp, vp, vp]
    assert list(L.xr_batch_tree_backup.argtypes) == [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    hdr = open(os.path.join(ROOT, "include", "xroute_hip.h")).read()
    assert "int32_t xr_batch_tree_open(xr_batch* b, int32_t group, int32_t n_par, int32_t node_cap, double c_init, double c_base," in hdr
    assert "int32_t xr_batch_tree_leaves(xr_batch* b, int32_t group, uint8_t* rows_out_dev, int64_t row_bytes, int32_t region_base," in hdr
    assert "int32_t xr_batch_tree_backup(xr_batch* b, int32_t group, const double* value_dev, const float* leaf_prior_dev," in hdr
    assert "#define XR_ABI_VERSION 9" in hdr and L.xr_abi_version() == 9          # an addition: the ABI version stays
    for name, val in (("XR_TREE_LEAF_TERMINAL", 1), ("XR_TREE_LEAF_FRESH", 2), ("XR_TREE_LEAF_NONE", 4)):
        assert getattr(_lib, name) == val and any(l.split()[:3] == ["#define", name, str(val)] for l in hdr.splitlines()), name
    assert (_lib.XR_TREE_LEAF_TERMINAL, _lib.XR_TREE_LEAF_FRESH, _lib.XR_TREE_LEAF_NONE) == (TERMINAL, FRESH, NONE)
    # the section is in its place: after the kept trees, before the guides
    k, s, m = hdr.index("---- kept trees"), hdr.index("---- evaluated tree search"), hdr.index("---- XR-Maze v2: global-route guides")
    assert k < s < m and hdr.count("---- evaluated tree search") == 1
    sec = " ".join(w for w in hdr[s:m].split() if w != "*")          # (the comment's line prefixes go)
    for phrase in ("XR-Tree v2, evaluated", "Own memory", "40 node_cap + 40 + n_par x (4 k_cap + 16) + 8 k_cap + 8 legal_words + 4",
                   "8 x (max_sims + 1)", "SNAPSHOT", "must re-open", "every access stays in bounds", "v1's Select rule word for word",
                   "XR_TREE_LEAF_TERMINAL", "XR_TREE_LEAF_FRESH", "XR_TREE_LEAF_NONE", "bit for bit what xr_batch_peek writes",
                   "keeps the line returns", "G = ret + v, one IEEE addition", "0.0 where that entry is not finite", "TERMINAL simulations only",
                   "strictly: the first wins", "S == 0 leaves the block as it is", "never given a new prior", "simulations so far",
                   "XR_PEEK_MAX", "XR_TREE_MAX_SIMS", "twice without a backup", "without pending leaves", "would pass max_sims",
                   "stream_per_region", "force_scratch_field", "NO TRACE", "ever synchronises", "Every message names the entry point",
                   "no Dirichlet noise", "no discounting", "no kept tree for this form"):
        assert phrase in sec, phrase
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "xr_batch_tree_open(vp, c_int, c_int, c_int, c_double, c_double, c_int, vp, c_int, vp)" in doc
    assert "xr_batch_tree_leaves(vp, c_int, vp, c_long, c_int, vp, vp, vp, vp, vp)" in doc
    assert "xr_batch_tree_backup(vp, c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp)" in doc


def test_product_library_links_the_three_kernels():
    L = _lib.lib()
    for name in ("xr_launch_tree_eval_open", "xr_launch_tree_eval_select", "xr_launch_tree_eval_backup"):
        assert hasattr(L, name), name


def test_null_arguments_without_gpu():
    L = _lib.lib()
    INV = _lib.XR_ERR_INVALID
    assert L.xr_batch_tree_open(None, -1, 2, 8, 1.25, 19652.0, 8, None, 4, None) == INV
    msg = L.xr_last_error()
    assert b"xr_batch_tree_open" in msg and b"null" in msg
    rows, out = (C.c_uint8 * 4096)(), (C.c_int32 * 64)()
    for args in ((None, -1, None, 64, 0, None, None, None, None, None), (None, -1, rows, 64, 0, out, None, None, None, None)):
        assert L.xr_batch_tree_leaves(*args) == INV
        msg = L.xr_last_error()
        assert b"xr_batch_tree_leaves" in msg and b"null" in msg
    v, vis, val, info = (C.c_double * 16)(), (C.c_int32 * 16)(), (C.c_double * 16)(), (C.c_int32 * 16)()
    for args in ((None, -1, None, None, None, None, None, None, None, None, None), (None, -1, v, None, vis, val, info, None, None, None, None)):
        assert L.xr_batch_tree_backup(*args) == INV
        msg = L.xr_last_error()
        assert b"xr_batch_tree_backup" in msg and b"null" in msg


def _bare_batch():
    import torch
    from xroute_env_amd.batch import RegionBatch
    rb = RegionBatch.__new__(RegionBatch)          # no handle, no library: whatever gets past the checks fails on the missing attributes
    rb.n_envs, rb.device, rb.legal_words, rb.k_max, rb.n_max = 10, torch.device("cpu"), 1, 5, 100
    rb._group_bounds = [0, 3, 10]
    return rb


def test_region_batch_checks_tree_open_arguments_before_the_library():
    import torch
    rb = _bare_batch()
    for kw, word in ((dict(n_par=0), "n_par"), (dict(n_par=_lib.XR_PEEK_MAX + 1, max_sims=_lib.XR_PEEK_MAX + 1), "n_par"), (dict(max_sims=1), "max_sims"),
                     (dict(max_sims=_lib.XR_TREE_MAX_SIMS + 1), "max_sims"), (dict(c_init=NAN), "c_init"), (dict(c_init=INF), "c_init"),
                     (dict(c_base=0.0), "c_base"), (dict(c_base=NAN), "c_base"), (dict(node_cap=0), "node_cap"), (dict(node_cap=2 ** 31), "node_cap"),
                     (dict(root_prior=torch.zeros((10, 5), dtype=torch.float64)), "root_prior"), (dict(root_prior=torch.zeros((9, 5))), "root_prior"),
                     (dict(root_prior=torch.zeros((10, 10))[:, ::2]), "root_prior"), (dict(root_prior=[[0.0] * 5] * 10), "root_prior"),
                     (dict(root_prior=torch.zeros((10, 5)), group=1), "root_prior"), (dict(group=2), "group")):
        with pytest.raises(ValueError, match=word):
            rb.tree_open(**dict(dict(n_par=2, max_sims=8), **kw))
    with pytest.raises(Exception) as ei:                                                              # a good one gets past the checks
        rb.tree_open(2, 8, root_prior=torch.zeros((7, 5)), group=1)
    assert "must be" not in str(ei.value) and not isinstance(ei.value, _lib.XRouteError), ei.value          # (none of the checks' own words)


def test_region_batch_checks_leaves_and_backup_arguments_before_the_library():
    import torch
    rb = _bare_batch()
    for fn, args in ((rb.tree_leaves, ()), (rb.tree_backup, (torch.zeros((10, 2), dtype=torch.float64),))):
        with pytest.raises(_lib.XRouteError) as ei:                                                   # no session: the library's own refusal
            fn(*args)
        assert ei.value.code == _lib.XR_ERR_STATE and "tree_open" in str(ei.value)
    rb._tree_sessions = {-1: 2, 1: 3}
    with pytest.raises(_lib.XRouteError):
        rb.tree_leaves(group=0)                                                                       # (that group has no session)
    need = 16 + 8 * (1 + 2)
    for kw, word in ((dict(row_bytes=need - 8), "row_bytes"), (dict(row_bytes=need + 4), "row_bytes"),
                     (dict(rows_out=torch.zeros((10, 2, need), dtype=torch.int8)), "rows_out"), (dict(rows_out=torch.zeros((10, 3, need), dtype=torch.uint8)), "rows_out"),
                     (dict(out=torch.zeros((10, 2, 8), dtype=torch.int64)), "out"), (dict(return_out=torch.zeros((10, 2), dtype=torch.float32)), "return_out"),
                     (dict(paths_out=torch.zeros((10, 2, 4), dtype=torch.int32)), "paths_out"), (dict(leaf_out=torch.zeros((10, 2, 3), dtype=torch.int32)), "leaf_out"),
                     (dict(leaf_out=torch.zeros((10, 2, 2), dtype=torch.int32), group=1), "leaf_out")):
        with pytest.raises(ValueError, match=word):
            rb.tree_leaves(**kw)
    f64, f32 = torch.float64, torch.float32
    for args, kw, word in (((torch.zeros((10, 2), dtype=f32),), {}, "value"), ((torch.zeros((10, 3), dtype=f64),), {}, "value"),
                           (([[0.0, 0.0]] * 10,), {}, "value"), ((torch.zeros((10, 4), dtype=f64)[:, ::2],), {}, "value"),
                           ((torch.zeros((10, 2), dtype=f64),), dict(group=1), "value"),
                           ((torch.zeros((10, 2), dtype=f64),), dict(leaf_prior=torch.zeros((10, 2, 5), dtype=f64)), "leaf_prior"),
                           ((torch.zeros((10, 2), dtype=f64),), dict(leaf_prior=torch.zeros((10, 2, 4), dtype=f32)), "leaf_prior"),
                           ((torch.zeros((10, 2), dtype=f64),), dict(leaf_prior=torch.zeros((10, 5), dtype=f32)), "leaf_prior")):
        with pytest.raises(ValueError, match=word):
            rb.tree_backup(*args, **kw)
    for call in (lambda: rb.tree_leaves(), lambda: rb.tree_backup(torch.zeros((7, 3), dtype=f64), torch.zeros((7, 3, 5), dtype=f32), group=1)):
        with pytest.raises(Exception) as ei:                                                          # good ones get past the checks
            call()
        assert "must be" not in str(ei.value) and not isinstance(ei.value, _lib.XRouteError), ei.value


def test_evaluated_search_checks_its_arguments():
    from xroute_env_amd.envs.tree_eval import evaluated_search
    rb = _bare_batch()
    with pytest.raises(ValueError, match="n_waves"):
        evaluated_search(rb, lambda *a, **k: None, 0, 2)
    with pytest.raises(ValueError, match="evaluate"):
        evaluated_search(rb, None, 2, 2)
    with pytest.raises(ValueError, match="n_par"):
        evaluated_search(rb, lambda *a, **k: None, 2, 0)


# ---- the twin on hand-made values ---------------------------------------------------------------------------------------------------
E = None


def _E():
    global E
    if E is None:
        E = _lib.tree_exploration_table(1.25, 19652.0, 256)
    return E


def _line(p):
    """The line return of path p: a different, non-dyadic number per path, so every addition rounds."""
    g = -1.0
    for d, n in enumerate(p):
        g = g - 0.1 * n / (d + 1.0)
    return g


def _val(p):
    return -0.37 * (len(p) + 1) - 0.01 * sum(p)


def _wave(sess, values=None, priors=None, value_fn=_val):
    """One leaves + backup on a session of one row.  values / priors: per lane, or None for value_fn / no prior."""
    paths, leaves = sess.leaves()
    nets = [[n for n in p if n] for p in paths[0]]
    lines = [_line(p) for p in nets]
    vals = [value_fn(p) for p in nets] if values is None else values
    res, G = sess.backup([lines], [vals], None if priors is None else [priors])
    return nets, leaves[0], lines, vals, res[0], G[0]


def test_the_open_call_builds_v1s_root_and_a_wave_follows_v1s_select():
    legal = [1, 2, 3, 5]
    prior = [0.5, 0.0, 1.5, 9.0, NAN]          # net 4 is not legal; NaN counts as 0
    sess = et.Session([legal], 3, 100, _E(), 12, 5, [prior])
    plain = tree_twin.RowTree(legal, 100, _E(), prior)
    t = sess.trees[0]
    assert [(n.net, n.P) for n in t.nodes] == [(n.net, n.P) for n in plain.nodes] == [(0, 1.0), (1, 0.25), (2, 0.0), (3, 0.75), (5, 0.0)]
    paths, leaves = sess.leaves()
    assert [p[:2] for p in paths[0]] == [[n for n in p] + [0] * (2 - len(p)) for p in plain.select(3)]          # v1's lanes, pending visits included
    assert all(f == FRESH for _, f in leaves[0]) and [t.nodes[i].net for i, _ in leaves[0]] == [[n for n in p if n][-1] for p in paths[0]]
    # a fresh block takes its P from the open call's row prior under v1's rule: below net 1 the legal nets are 2, 3, 5
    first = t.nodes[leaves[0][0][0]]
    assert [(t.nodes[i].net, t.nodes[i].P) for i in range(first.first, first.first + first.count)] == [(2, 0.0), (3, 1.0), (5, 0.0)]


def test_a_terminal_leaf_ignores_its_value_and_only_terminal_lines_are_best():
    legal = [2, 7]
    sess = et.Session([legal], 2, 50, _E(), 40, 7)
    seen_terminal = 0
    for w in range(6):
        paths, leaves = sess.leaves()
        nets = [[n for n in p if n] for p in paths[0]]
        lines = [_line(p) for p in nets]
        before = sess.trees[0].best
        # poison the value of every terminal lane: it must not be read; the others get a huge value that must not become the best line
        vals = [NAN if f & TERMINAL else 1000.0 for _, f in leaves[0]]
        res, G = sess.backup([lines], [vals])
        for j, (_, f) in enumerate(leaves[0]):
            if f & TERMINAL:
                seen_terminal += 1
                assert len(nets[j]) == 2 and G[0][j] == lines[j]
            else:
                assert G[0][j] == lines[j] + 1000.0
        terminal_G = [G[0][j] for j, (_, f) in enumerate(leaves[0]) if f & TERMINAL]
        assert res[0]["best_return"] == max([before] + terminal_G) and res[0]["best_return"] < 0.0
        if terminal_G:
            assert sorted(n for n in res[0]["best_order"] if n) == legal
    assert seen_terminal > 0
    t = sess.trees[0]
    assert t.mx > 900.0 and t.best < 0.0          # max follows every G, best only the terminal ones
    # strictly greater: the first of two equal terminal lines stays
    sess = et.Session([[1, 2]], 1, 50, _E(), 40, 2)
    orders = []
    for w in range(8):
        paths, leaves = sess.leaves()
        res, _ = sess.backup([[-5.0]], [[0.0]])
        if leaves[0][0][1] & TERMINAL:
            orders.append(([n for n in paths[0][0] if n], list(res[0]["best_order"])))
    assert len(orders) >= 2 and all(o[1] == orders[0][0] for o in orders) and len({tuple(o[0]) for o in orders}) == 2


def test_values_that_are_not_finite_count_as_zero():
    legal = [1, 2, 3]
    for bad in (NAN, INF, -INF):
        a = et.Session([legal], 2, 50, _E(), 8, 3)
        b = et.Session([legal], 2, 50, _E(), 8, 3)
        for w in range(3):
            _, _, lines, _, ra, Ga = _wave(a, values=[bad, -0.25])
            _, _, _, _, rb, Gb = _wave(b, values=[0.0, -0.25])
            assert Ga == Gb and ra == rb and Ga[0] == lines[0]
        assert all(x == x and abs(x) < INF for n in a.trees[0].nodes for x in (n.W,))


def test_a_prior_row_without_weight_leaves_the_block_as_it_is():
    legal = [1, 2, 3, 4]
    root_prior = [1.0, 2.0, 3.0, 4.0]
    for row in ([0.0] * 4, [NAN] * 4, [-1.0, -2.0, -INF, -0.5], [NAN, -1.0, 0.0, INF]):
        sess = et.Session([legal], 2, 50, _E(), 8, 4, [root_prior])
        ref = et.Session([legal], 2, 50, _E(), 8, 4, [root_prior])
        _wave(sess, priors=[row, row])
        _wave(ref)
        t, r = sess.trees[0], ref.trees[0]
        assert t.repriored == 0 and [(n.net, n.P) for n in t.nodes] == [(n.net, n.P) for n in r.nodes], row
    # and one with weight replaces the block: P = w / S over the block's nets alone
    sess = et.Session([legal], 1, 50, _E(), 8, 4, [root_prior])
    nets, leaves, *_ = _wave(sess, priors=[[5.0, 1.0, NAN, 3.0]])
    t = sess.trees[0]
    blk = t.nodes[leaves[0][0]]
    got = {t.nodes[i].net: t.nodes[i].P for i in range(blk.first, blk.first + blk.count)}
    assert nets[0] == [1] and got == {2: 1.0 / 4.0, 3: 0.0, 4: 3.0 / 4.0} and t.repriored == 1          # (net 1's weight is not in S)


def test_a_leaf_that_is_not_fresh_is_never_given_a_new_prior():
    # a pool with room for the root's block and one more: the second lane's leaf stays unexpanded (flags 0), and is selected again later
    legal = [1, 2, 3]
    sess = et.Session([legal], 2, 1 + 3 + 2, _E(), 20, 3)
    t = sess.trees[0]
    heavy = [9.0, 9.0, 1.0]
    snap = None
    stale = 0
    for w in range(5):
        paths, leaves = sess.leaves()
        lines = [_line([n for n in p if n]) for p in paths[0]]
        stale += sum(1 for _, f in leaves[0] if not f & FRESH)
        if w == 1:
            snap = [(n.net, n.P) for n in t.nodes]
        sess.backup([lines], [[-0.5, -0.5]], [[heavy, heavy]] if w >= 1 else None)
        if w >= 1:
            assert [(n.net, n.P) for n in t.nodes] == snap, w
    assert stale >= 8 and t.flags == FULL and t.repriored == 0
    # a terminal leaf has no block either
    sess = et.Session([[4]], 1, 10, _E(), 4, 4)
    for w in range(3):
        paths, leaves = sess.leaves()
        assert leaves[0][0][1] == TERMINAL and paths[0][0] == [4, 0, 0, 0]
        sess.backup([[-1.0]], [[NAN]], [[[1.0, 1.0, 1.0, 1.0]]])
    assert sess.trees[0].repriored == 0 and sess.trees[0].nodes[1].N == 3


def test_a_full_pool():
    legal = [1, 2, 3]
    # node_cap 1: the root cannot be expanded; every lane's leaf is the root, with flags 0, and every path is empty
    sess = et.Session([legal], 2, 1, _E(), 4, 3)
    for w in range(2):
        nets, leaves, lines, vals, res, G = _wave(sess)
        assert nets == [[], []] and leaves == [[0, 0], [0, 0]] and G == [lines[0] + vals[0]] * 2
    assert res["info"] == [4, 1, 0, FULL] and res["visits"] == [0, 0, 0] and res["value"] == [-INF] * 3
    assert res["best_return"] == -INF and res["best_order"] == [0, 0, 0]          # no terminal simulation: no best line
    assert sess.trees[0].nodes[0].N == 4 and sess.trees[0].nodes[0].V == 0
    # node_cap K + 1: the root's block fits and nothing else
    sess = et.Session([legal], 2, 4, _E(), 6, 3)
    for w in range(3):
        nets, leaves, _, _, res, _ = _wave(sess)
        assert all(len(p) == 1 and f == 0 for p, (_, f) in zip(nets, leaves))
    assert res["info"] == [6, 4, 1, FULL] and sum(res["visits"]) == 6 and len(sess.trees[0].nodes) == 4


def test_done_rows_and_the_call_order():
    sess = et.Session([[], [1, 2]], 2, 20, _E(), 4, 2)
    paths, leaves = sess.leaves()
    assert paths[0] == [[0, 0], [0, 0]] and leaves[0] == [[-1, NONE], [-1, NONE]]
    with pytest.raises(RuntimeError):
        sess.leaves()                                             # twice without a backup
    res, G = sess.backup([[0.0, 0.0], [-1.0, -2.0]], [[5.0, 5.0], [0.5, 0.5]])
    assert res[0] == dict(visits=[0, 0], value=[-INF, -INF], info=[0, 0, 0, 0], best_order=[0, 0], best_return=-INF) and G[0] == [0.0, 0.0]
    assert res[1]["info"][0] == 2 and G[1] == [-0.5, -1.5]
    with pytest.raises(RuntimeError):
        sess.backup([[0.0, 0.0]] * 2, [[0.0, 0.0]] * 2)            # without pending leaves
    sess.leaves()
    sess.backup([[0.0, 0.0]] * 2, [[0.0, 0.0]] * 2)
    with pytest.raises(OverflowError):
        sess.leaves()                                             # a wave that would pass max_sims
    with pytest.raises(ValueError):
        et.Session([[1]], 3, 20, _E(), 2, 1)                      # max_sims below n_par


def test_host_code_under_asan_ubsan_as_a_program_of_its_own():
    r = subprocess.run(["make", "-C", HOSTSAN, "tree_eval_args"], capture_output=True, text=True)
    assert r.returncode == 0, "build of the evaluated-tree argument program failed: " + r.stderr[-1500:]
    assert "warning" not in r.stderr, r.stderr[-1500:]
    out = subprocess.run([os.path.join(HOSTSAN, "tree_eval_args")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("TREE_EVAL_ARGS_OK "), (out.stdout[-1500:], out.stderr[-3000:])
    assert out.stderr == "", out.stderr[-3000:]
