"""Kept evaluated trees (xr_batch_tree_reopen, "XR-Tree v2, kept") without a GPU: the entry point is exported, bound, declared in its
place and present in the INTEGRATION stub; null and invalid arguments are refused without a device; RegionBatch.tree_open(keep=...,
played=...) checks its arguments before the library; the spec's twin (tests/tree_eval_keep_twin.py) on hand-made values — the re-rooted
numbering and W' = W - N * r, played == 0, every rebuild reason, carried priors, done rows, the best line; and the host C++ under ASan +
UBSan as a program of its own (tests/hostsan_tree_eval_keep/tree_eval_keep_args.cpp), its trace compared with the committed one."""
import ctypes as C
import os
import subprocess

import pytest

from tests import tree_eval_keep_twin as ekt
from tests import tree_eval_twin as et
from tests import tree_twin
from tests.tree_keep_twin import State
from xroute_env_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSAN = os.path.join(ROOT, "tests", "hostsan_tree_eval_keep")
INF = float("inf")
NAN = float("nan")
KEPT, FULL, MAX = ekt.KEPT, tree_twin.POOL_FULL, ekt.MAX_SIMS
TERMINAL, FRESH = et.TERMINAL, et.FRESH
_TABLE = {}


def _E():
    if "E" not in _TABLE:
        _TABLE["E"] = _lib.tree_exploration_table(1.25, 19652.0, MAX)
    return _TABLE["E"]


# ---- the symbol ---------------------------------------------------------------------------------------------------------------------
def test_symbol_bound_typed_declared_and_in_the_stub():
    L = _lib.lib()
    vp, i32, f64 = C.c_void_p, C.c_int32, C.c_double
    assert "xr_batch_tree_reopen" in _lib.SYMBOLS and L.xr_batch_tree_reopen.restype is i32
    assert list(L.xr_batch_tree_reopen.argtypes) == [vp, i32, vp, i32, i32, f64, f64, i32, vp, i32, vp, vp]
    hdr = open(os.path.join(ROOT, "include", "xroute_hip.h")).read()
    assert "int32_t xr_batch_tree_reopen(xr_batch* b, int32_t group, const int32_t* played_dev," in hdr
    assert "#define XR_ABI_VERSION 9" in hdr and L.xr_abi_version() == 9          # an addition: the ABI version stays
    assert _lib.XR_TREE_KEPT == KEPT and hdr.count("#define XR_TREE_KEPT 2") == 1
    # the section is in its place: after the evaluated search, before the guides
    s, k, m = hdr.index("---- evaluated tree search"), hdr.index("---- kept evaluated trees"), hdr.index("---- XR-Maze v2: global-route guides")
    assert s < k < m and hdr.count("---- kept evaluated trees") == 1
    sec = " ".join(w for w in hdr[k:m].split() if w != "*")
    for phrase in ("XR-Tree v2, kept", "every message names xr_batch_tree_reopen", "KEYED", "there is no second copy", "is not keyed",
                   "played == NULL", "leaves waiting for a backup", "node_cap, k_cap, legal_words or n_par", "xr_batch_set_groups or xr_batch_load_regions",
                   "N + max_sims <= XR_TREE_MAX_SIMS", "env_steps == key.env_steps + 1", "A rebuild is never an error", "net = 0 and P = 1.0",
                   "breadth-first compaction", "W' = W - (double)N", "contraction off", "V is 0", "min' = min - r and max' = max - r",
                   "XR_TREE_KEPT alone", "never FRESH again", "kept {0, 0}", "E[0 .. XR_TREE_MAX_SIMS]", "never clamps at a carried root",
                   "THIS session's simulations", "{N of the new root before this session's simulations, nodes carried}",
                   "80 node_cap + 40 + n_par x (4 k_cap + 16) + 8 k_cap + 8 legal_words + 4 + 24", "eleven arrays", "8 x (XR_TREE_MAX_SIMS + 1)",
                   "has nothing to keep and rebuilds every row", "the best line does not carry", "at most one real route", "xr_batch_branch",
                   "forfeits the tree"):
        assert phrase in sec, phrase
    open_sec = " ".join(w for w in hdr[s:k].split() if w != "*")
    assert "xr_batch_tree_reopen" in open_sec and "is not keyed" in open_sec          # the open section points here
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "xr_batch_tree_reopen(vp, c_int, vp, c_int, c_int, c_double, c_double, c_int, vp, c_int, vp, vp)" in doc


def test_product_library_links_the_reopen_kernel():
    assert hasattr(_lib.lib(), "xr_launch_tree_eval_reopen")


def test_null_and_invalid_arguments_without_gpu():
    L = _lib.lib()
    played, kept = (C.c_int32 * 8)(), (C.c_int32 * 16)()
    for args in ((None, -1, None, 2, 8, 1.25, 19652.0, 8, None, 4, None, None), (None, -1, played, 0, 0, NAN, -1.0, 0, None, 0, kept, None)):
        assert L.xr_batch_tree_reopen(*args) == _lib.XR_ERR_INVALID
        msg = L.xr_last_error()
        assert b"xr_batch_tree_reopen" in msg and b"null" in msg
    cfg = _lib.default_config()
    cfg.n_envs = 2
    h = C.c_void_p()
    if L.xr_batch_create(C.byref(cfg), C.byref(h)) == 0:          # (a batch without regions needs no device on some hosts; none: skip the rest)
        try:
            assert L.xr_batch_tree_reopen(h, -1, played, 2, 8, 1.25, 19652.0, 8, None, 4, kept, None) == _lib.XR_ERR_STATE
            assert b"xr_batch_tree_reopen: load regions first" in L.xr_last_error()
        finally:
            L.xr_batch_destroy(h)


def _bare_batch():
    import torch
    from xroute_env_amd.batch import RegionBatch
    rb = RegionBatch.__new__(RegionBatch)          # no handle, no library: whatever gets past the checks fails on the missing attributes
    rb.n_envs, rb.device, rb.legal_words, rb.k_max, rb.n_max = 10, torch.device("cpu"), 1, 5, 100
    rb._group_bounds = [0, 3, 10]
    return rb


def test_region_batch_checks_reopen_arguments_before_the_library():
    import torch
    rb = _bare_batch()
    i32 = torch.int32
    with pytest.raises(ValueError, match="played needs keep"):
        rb.tree_open(2, 8, played=torch.zeros(10, dtype=i32))
    for kw, word in ((dict(played=torch.zeros(10, dtype=torch.int64)), "played"), (dict(played=torch.zeros(9, dtype=i32)), "played"),
                     (dict(played=torch.zeros((10, 1), dtype=i32)), "played"), (dict(played=torch.zeros(20, dtype=i32)[::2]), "played"),
                     (dict(played=[0] * 10), "played"), (dict(played=torch.zeros(10, dtype=i32), group=1), "played"),
                     (dict(n_par=0), "n_par"), (dict(max_sims=1), "max_sims"), (dict(max_sims=MAX + 1), "max_sims"), (dict(c_init=NAN), "c_init"),
                     (dict(c_base=0.0), "c_base"), (dict(node_cap=0), "node_cap"), (dict(root_prior=torch.zeros((9, 5))), "root_prior")):
        with pytest.raises(ValueError, match=word):
            rb.tree_open(**dict(dict(n_par=2, max_sims=8, keep=True), **kw))
    for kw in (dict(played=torch.zeros(7, dtype=i32), group=1), dict(), dict(played=torch.zeros(10, dtype=i32), root_prior=torch.zeros((10, 5)))):
        with pytest.raises(Exception) as ei:                                                          # good ones get past the checks
            rb.tree_open(2, 8, keep=True, **kw)
        assert "must be" not in str(ei.value) and "needs" not in str(ei.value) and not isinstance(ei.value, _lib.XRouteError), ei.value
    from xroute_env_amd.envs.tree_eval import evaluated_search
    with pytest.raises(ValueError, match="played needs keep"):
        evaluated_search(rb, lambda *a, **k: None, 2, 2, played=torch.zeros(10, dtype=i32))


# ---- the twin on hand-made values ---------------------------------------------------------------------------------------------------
def _line(p):
    """The line return of path p: a different, non-dyadic number per path, so every addition rounds."""
    g = -1.0
    for d, n in enumerate(p):
        g = g - 0.1 * n / (d + 1.0)
    return g


def _val(p):
    return -0.37 * (len(p) + 1) - 0.01 * sum(p)


def _waves(sess, n, priors=None):
    """n waves on a session of one row; priors: None, or a function (path) -> a prior row.  Returns the last result."""
    res = None
    for _ in range(n):
        paths, leaves = sess.leaves()
        nets = [[v for v in p if v] for p in paths[0]]
        res, _ = sess.backup([[_line(p) for p in nets]], [[_val(p) for p in nets]], None if priors is None else [[priors(p) for p in nets]])
    return res[0]


def _searched(legal, waves=4, n_par=3, cap=200, steps=3, region=2, replay=1, priors=None, k_cap=8):
    """A pool whose row has searched State(steps, region, replay, legal): (pool, the state, the last result)."""
    pool = ekt.KeyedPool()
    st = State(steps, region, replay, legal)
    sess, kept = pool.reopen([st], None, n_par, cap, _E(), (waves + 1) * n_par, k_cap)          # (room for one wave more)
    assert kept == [[0, 0]]
    return pool, st, _waves(sess, waves, priors)


def _nodes(t):
    return [(n.net, n.N, n.V, n.W, n.P, n.first, n.count) for n in t.nodes]


def _most_visited(res):
    return max(range(len(res["visits"])), key=lambda i: (res["visits"][i], -i)) + 1


def test_re_rooting_numbers_the_nodes_breadth_first_and_shifts_every_return_by_the_reward():
    legal = [1, 2, 3, 5]
    pool, st, res = _searched(legal, priors=lambda p: [3.0, 1.0, 2.0, 0.0, 5.0, 0.0, 0.0, 0.0])
    old = pool.rows[0].tree
    a = _most_visited(res)
    r = -1.7
    child = next(i for i in range(old.nodes[0].first, old.nodes[0].first + old.nodes[0].count) if old.nodes[i].net == a)
    assert old.nodes[child].first >= 0 and old.nodes[child].N >= 3
    after = State(st.env_steps + 1, st.region, st.replay, [n for n in legal if n != a], r)
    sess, kept = pool.reopen([after], [a], 3, 200, _E(), 12, 8)
    new = sess.trees[0]
    # an independent walk: a queue of old indices, children appended in their old order
    order = [child]
    for i in order:
        o = old.nodes[i]
        if o.first >= 0:
            order += list(range(o.first, o.first + o.count))
    assert kept == [[old.nodes[child].N, len(order)]] and len(new.nodes) == len(order) and len(order) > 1 + len(after.legal)
    where = {o: i for i, o in enumerate(order)}
    for i, o in enumerate(order):
        src, nd = old.nodes[o], new.nodes[i]
        nr = float(src.N) * r
        assert nd.W == src.W - nr and nd.N == src.N and nd.V == 0 and nd.count == src.count, i
        assert (nd.net, nd.P) == ((0, 1.0) if i == 0 else (src.net, src.P)), i
        assert nd.first == (where[src.first] if src.first >= 0 else -1), i
    assert (new.mn, new.mx) == (old.mn - r, old.mx - r) and new.flags == KEPT and new.best == -INF and new.max_depth == 0 and new.sims == 0
    assert any(n.P not in (1.0, 1.0 / 3.0, 0.5) for n in new.nodes[1:])          # P values an evaluator's prior gave
    res2 = _waves(sess, 4)
    assert res2["info"][0] == 12 and res2["info"][3] == KEPT and sum(res2["visits"]) == kept[0][0] - 1 + 12
    assert new.nodes[0].N == kept[0][0] + 12


def test_played_zero_keeps_the_whole_tree_and_counts_this_sessions_simulations():
    pool, st, res = _searched([1, 2, 3])
    before = _nodes(pool.rows[0].tree)
    sess, kept = pool.reopen([st], [0], 3, 200, _E(), 6, 8)
    t = sess.trees[0]
    assert kept == [[12, len(before)]] and _nodes(t) == before and t.flags == KEPT and t.sims == 0 and t.best == -INF
    res2 = _waves(sess, 2)
    assert res2["info"][0] == 6 and sum(res2["visits"]) == 18 and res2["info"][3] == KEPT
    with pytest.raises(OverflowError):
        sess.leaves()          # max_sims bounds this session's simulations


def _rebuilt(pool, st, played, what, max_sims=12, cap=200, n_par=3, k_cap=8, **kw):
    sess, kept = pool.reopen([st], played, n_par, cap, _E(), max_sims, k_cap, **kw)
    fresh = et.EvalRowTree(st.legal, cap, _E())
    t = sess.trees[0]
    assert kept == [[0, 0]] and _nodes(t) == _nodes(fresh) and t.flags == 0 and (t.mn, t.mx) == (INF, -INF), what
    return sess


def test_every_rebuild_reason():
    legal = [1, 2, 3, 5]
    def after(a, **kw):
        base = dict(env_steps=4, region=2, replay=1, legal=[n for n in legal if n != a], reward=-0.5)
        base.update(kw)
        return State(**base)
    cases = []
    pool, st, res = _searched(legal)
    a = _most_visited(res)
    other = next(n for n in legal if n != a)
    cases += [("a wrong net", after(a), [other]), ("a negative entry", after(a), [-1]), ("a net that was never legal", after(a), [4]),
              ("a net beyond the words", after(a), [200]), ("no step", st, [a]), ("two steps", after(a, env_steps=5), [a]),
              ("played 0 after a step", after(a), [0]), ("another region", after(a, region=3), [a]), ("another replay", after(a, replay=0), [a]),
              ("one legal bit more", after(a, legal=sorted([n for n in legal if n != a] + [4])), [a]),
              ("one legal bit less", after(a, legal=[n for n in legal if n != a][1:]), [a]),
              ("played 0, one legal bit off", State(3, 2, 1, legal[:-1]), [0])]
    for what, state, played in cases:
        pool, st, res = _searched(legal)
        assert _most_visited(res) == a
        _rebuilt(pool, state, played, what)
        # ... and the same pool keeps the row when told the truth
        pool, st, res = _searched(legal)
        sess, kept = pool.reopen([after(a)], [a], 3, 200, _E(), 12, 8)
        assert kept[0][0] > 0 and sess.trees[0].flags == KEPT, what
    # an unexpanded root (the pool had no room for its block) and a missing child (a damaged block)
    pool = ekt.KeyedPool()
    sess, _ = pool.reopen([st], None, 3, 1, _E(), 12, 8)
    assert sess.trees[0].nodes[0].first < 0 and sess.trees[0].flags == FULL
    _waves(sess, 2)
    sess, kept = pool.reopen([after(a)], [a], 3, 1, _E(), 12, 8)
    assert kept == [[0, 0]] and sess.trees[0].flags == FULL          # rebuilt, and as full as a fresh tree of one node
    pool, st, res = _searched(legal)
    root = pool.rows[0].tree.nodes[0]
    for i in range(root.first, root.first + root.count):
        if pool.rows[0].tree.nodes[i].net == a:
            pool.rows[0].tree.nodes[i].net = 4
    _rebuilt(pool, after(a), [a], "a missing child")
    # the host's reasons: un-keyed, pending, each shape field
    pool, st, res = _searched(legal)
    pool.open([after(a).legal], 3, 200, _E(), 12, 8)
    _rebuilt(pool, after(a), [a], "un-keyed: an open session in between")
    pool, st, res = _searched(legal)
    pool.session.leaves()
    _rebuilt(pool, st, [0], "pending: leaves without a backup")
    pool, st, res = _searched(legal)
    pool.invalidate()
    _rebuilt(pool, after(a), [a], "set_groups in between")
    for what, kw in (("node_cap", dict(cap=201)), ("n_par", dict(n_par=2)), ("k_cap", dict(k_cap=9)), ("lo", dict(lo=1)), ("legal_words", dict(legal_words=2))):
        pool, st, res = _searched(legal)
        _rebuilt(pool, after(a), [a], what, **kw)
    pool, st, res = _searched(legal)
    sess, kept = pool.reopen([after(a), after(a)], [a, a], 3, 200, _E(), 12, 8)
    assert kept == [[0, 0], [0, 0]]                                   # rows
    pool, st, res = _searched(legal)
    sess, kept = pool.reopen([after(a)], [a], 3, 200, _E(), 30, 8, priors=[[1.0] * 8])
    assert kept[0][0] > 0                                             # max_sims and the prior may differ


def test_the_simulation_budget_at_exactly_the_limit_and_one_above():
    legal = [1, 2, 3]
    pool, st, res = _searched(legal)
    sess, kept = pool.reopen([st], [0], 3, 200, _E(), MAX - 12, 8)
    assert kept[0][0] == 12 and sess.trees[0].flags == KEPT
    _rebuilt(pool, st, [0], "the root's N + max_sims one above", max_sims=MAX - 12 + 1)
    pool, st, res = _searched(legal)
    a = _most_visited(res)
    n = res["visits"][a - 1]
    after = State(st.env_steps + 1, st.region, st.replay, [x for x in legal if x != a], -2.0)
    sess, kept = pool.reopen([after], [a], 3, 200, _E(), MAX - n, 8)
    assert kept[0][0] == n and sess.trees[0].flags == KEPT
    # the table reaches the counts a carried root can meet: a wave at the limit selects without clamping
    assert len(_E()) == MAX + 1
    pool, st, res = _searched(legal)
    _rebuilt(pool, after, [a], "the child's N + max_sims one above", max_sims=MAX - n + 1)


def test_a_carried_block_keeps_its_leaf_prior_and_is_never_repriored():
    legal = [1, 2, 3, 4]
    first = lambda p: [1.0, 2.0, 3.0, 4.0, 0.0, 0.0, 0.0, 0.0]
    pool, st, res = _searched(legal, priors=first)
    assert pool.rows[0].tree.repriored > 0
    a = _most_visited(res)
    after = State(st.env_steps + 1, st.region, st.replay, [x for x in legal if x != a], -0.3)
    sess, kept = pool.reopen([after], [a], 3, 200, _E(), 12, 8, priors=[[9.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0]])
    t = sess.trees[0]
    carried = kept[0][1]
    snap = [(n.net, n.P) for n in t.nodes[:carried]]
    root = t.nodes[0]
    left = [x for x in legal if x != a]
    S = sum(first(None)[x - 1] for x in left)
    assert [t.nodes[i].P for i in range(root.first, root.first + root.count)] == [first(None)[x - 1] / S for x in left]          # the evaluator's P, carried
    heavy = lambda p: [0.0, 0.0, 0.0, 7.0, 0.0, 0.0, 0.0, 0.0]
    _waves(sess, 4, priors=heavy)
    assert [(n.net, n.P) for n in t.nodes[:carried]] == snap          # no carried node's P moved, expanded block or not ...
    assert len(t.nodes) > carried and t.repriored > 0                 # ... while the blocks this session made took the evaluator's prior
    # a carried leaf that is expanded in this session is FRESH then, under this call's row prior until its lane's leaf prior lands
    assert t.sims == 12


def test_done_rows():
    pool = ekt.KeyedPool()
    states = [State(0, 0, 0, []), State(0, 1, 0, [2])]
    sess, kept = pool.reopen(states, None, 2, 20, _E(), 4, 2)
    assert kept == [[0, 0], [0, 0]]
    paths, leaves = sess.leaves()
    assert leaves[0] == [[-1, et.NONE]] * 2 and leaves[1][0][1] == TERMINAL          # (one net: its child is terminal)
    res, _ = sess.backup([[0.0, 0.0], [-1.0, -1.0]], [[0.0, 0.0], [0.5, 0.5]])
    assert res[0] == dict(visits=[0, 0], value=[-INF, -INF], info=[0, 0, 0, 0], best_order=[0, 0], best_return=-INF)
    # the played net was the last: a done row, kept {0, 0}, although its key agrees
    after = [State(0, 0, 0, []), State(1, 1, 0, [], -3.0)]
    sess, kept = pool.reopen(after, [0, 2], 2, 20, _E(), 4, 2)
    assert kept == [[0, 0], [0, 0]] and sess.trees[1].done and sess.trees[1].flags == 0
    paths, leaves = sess.leaves()
    res, G = sess.backup([[0.0, 0.0]] * 2, [[1.0, 1.0]] * 2)
    assert res[1] == res[0] and G == [[0.0, 0.0]] * 2


def test_the_best_line_does_not_carry():
    pool, st, res = _searched([2, 7], waves=4, n_par=2)
    assert res["best_return"] > -INF and sorted(n for n in res["best_order"] if n) == [2, 7]
    sess, kept = pool.reopen([st], [0], 2, 200, _E(), 2, 8)
    assert kept[0][0] == 8 and sess.trees[0].best == -INF and sess.trees[0].best_order is None
    paths, leaves = sess.leaves()
    res2, G = sess.backup([[-9.0, -9.0]], [[0.0, 0.0]])
    terminal = [g for g, (_, f) in zip(G[0], leaves[0]) if f & TERMINAL]
    assert res2[0]["best_return"] == max([-INF] + terminal)          # this session's terminal simulations alone: -9 at the best, not the first session's
    a = _most_visited(res)
    pool, st, res = _searched([2, 7], waves=4, n_par=2)
    after = State(st.env_steps + 1, st.region, st.replay, [n for n in (2, 7) if n != a], -1.0)
    sess, kept = pool.reopen([after], [a], 2, 200, _E(), 2, 8)
    assert sess.trees[0].best == -INF and sess.trees[0].best_order is None and kept[0][0] > 0


def test_an_episode_in_the_twin_meets_the_gpu_tests_conditions():
    """What tests/test_gpu_tree_eval_keep.py asks of its episode, on the CPU with hand-made values: for net counts 1, 2, 5, 5, 3 at 4 x 3
    simulations per ply every stepped row with a net left is kept, carries its played child's block, and shows the carried visits."""
    counts = (1, 2, 5, 5, 3)
    states = [State(0, r, 0, list(range(1, k + 1))) for r, k in enumerate(counts)]
    pool = ekt.KeyedPool()
    played, kept_plies, seen_n, seen_nodes = None, 0, [], []
    for ply in range(6):
        if not any(s.legal for s in states):
            break
        sess, kept = pool.reopen(states, played, 3, 1 + 4 * 13 * 5, _E(), 12, 5)
        for _ in range(4):
            paths, _ = sess.leaves()
            nets = [[[v for v in p if v] for p in row] for row in paths]
            res, _ = sess.backup([[_line(p) - 0.01 * r for p in row] for r, row in enumerate(nets)], [[_val(p) for p in row] for row in nets])
        if played is not None:
            must = [r for r, s in enumerate(states) if s.legal and played[r] > 0]
            for r in must:
                assert sess.trees[r].flags == KEPT and kept[r][1] >= 1 + len(states[r].legal) and sum(res[r]["visits"]) == kept[r][0] - 1 + 12, (ply, r)
                seen_n.append(kept[r][0]); seen_nodes.append(kept[r][1])
            kept_plies += bool(must)
        played = [_most_visited(res[r]) if s.legal else 0 for r, s in enumerate(states)]
        states = [State(s.env_steps + (1 if played[r] else 0), s.region, s.replay, [n for n in s.legal if n != played[r]], -0.5 * played[r]) for r, s in enumerate(states)]
    assert kept_plies >= 4 and min(seen_n) >= 1 and max(seen_nodes) > 5


# ---- the host C++ under the sanitizers ------------------------------------------------------------------------------------------------
def test_host_code_under_asan_ubsan_as_a_program_of_its_own_and_its_trace():
    r = subprocess.run(["make", "-C", HOSTSAN, "tree_eval_keep_args"], capture_output=True, text=True)
    assert r.returncode == 0, "build of the reopen argument program failed: " + r.stderr[-1500:]
    assert "warning" not in r.stderr, r.stderr[-1500:]
    out = subprocess.run([os.path.join(HOSTSAN, "tree_eval_keep_args")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.splitlines()[-1].startswith("TREE_EVAL_KEEP_ARGS_OK "), (out.stdout[-1500:], out.stderr[-3000:])
    assert out.stderr == "", out.stderr[-3000:]
    want = open(os.path.join(HOSTSAN, "tree_eval_keep_args.expected")).read()
    got = out.stdout
    if got != want:
        gl, wl = got.splitlines(), want.splitlines()
        first = next((i for i, (x, y) in enumerate(zip(gl, wl)) if x != y), min(len(gl), len(wl)))
        raise AssertionError(f"the trace differs from tree_eval_keep_args.expected at line {first + 1}: got {gl[first:first + 1]}, expected {wl[first:first + 1]}")
    # what the trace has to show, by name: both directions of the half flip, played reaching the launcher and NULL reaching it, the table
    assert "new=half1 old=half0 played=caller" in want and "new=half0 old=half1 played=caller" in want and "played=NULL" in want
    assert "a table of 65537 entries" in want and "carve nodes=0 old_nodes=12800 rs=25600" in want
