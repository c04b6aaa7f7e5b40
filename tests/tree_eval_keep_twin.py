""""XR-Tree v2, kept" (include/xroute_hip.h, "---- kept evaluated trees") as plain Python: the twin of xr_batch_tree_reopen for the tests.
The tree of a row is tests/tree_eval_twin.EvalRowTree; the key (State), the node shift (shifted) and the per-row mode decision
(KeptRow._mode) are tests/tree_keep_twin's — all imported, not edited.  What is this file's own: a keyed row whose begin() re-roots an
EvalRowTree, the caller's pool with the host's rebuild rule (un-keyed, pending, shape), and a Session over given trees whose leaves() /
backup() are the evaluated twin's.  Line returns, values and priors stay arguments, so the same code runs on hand-made numbers without
a GPU (tests/test_tree_eval_keep_host.py) and beside the device session (tests/test_gpu_tree_eval_keep.py)."""
import copy

from tests import tree_eval_twin as et
from tests import tree_keep_twin as kt
from tests.tree_keep_twin import KEPT, MAX_SIMS, State, shifted

assert KEPT == 2 and MAX_SIMS == 65536


class KeyedRow(kt.KeptRow):
    """One row of a keyed pool: the tree of the last session and the State it was keyed to."""

    def begin(self, st, played, max_sims, node_cap, E, prior=None):
        """The reopen kernel for this row: (the EvalRowTree the new session searches in, kept = [N of the new root, nodes carried])."""
        mode, child = self._mode(st, played, max_sims)
        old = self.tree
        tree = et.EvalRowTree(st.legal, node_cap, E, prior)          # mode 0: exactly what the open call builds
        kept = [0, 0]
        if mode == 1:
            tree.nodes = [copy.copy(n) for n in old.nodes]
            tree.mn, tree.mx = old.mn, old.mx
            tree.flags = KEPT
            kept = [old.nodes[0].N, len(old.nodes)]
        elif mode == 2:
            r = st.reward
            root = shifted(old.nodes[child], r)
            root.P, root.net = 1.0, 0
            nodes, src = [root], [child]
            i = 0
            while i < len(nodes):          # the new nodes in index order: the children block of every expanded one is appended
                o = old.nodes[src[i]]
                if o.first >= 0:
                    nodes[i].first = len(nodes)
                    for c in range(o.first, o.first + o.count):
                        nodes.append(shifted(old.nodes[c], r))
                        src.append(c)
                i += 1
            tree.nodes = nodes
            tree.mn, tree.mx = old.mn - r, old.mx - r
            tree.flags = KEPT
            kept = [root.N, len(nodes)]
        if mode and tree.nodes[0].first < 0:          # an unexpanded root: this call's prior
            tree._expand(0, [])
        self.tree = tree
        self.key = State(st.env_steps, st.region, st.replay, st.legal)
        return tree, kept


class Session(et.Session):
    """A session over given trees: leaves() / backup() and the call-order rules are the evaluated twin's.  max_sims bounds this
    session's simulations; info[0] of a result is this session's count (a tree's `sims` starts at 0 in begin())."""

    def __init__(self, trees, n_par, max_sims, k_cap):
        if not 1 <= n_par <= max_sims:
            raise ValueError("max_sims below n_par")
        self.trees = trees
        self.n_par, self.max_sims, self.k_cap = n_par, max_sims, k_cap
        self.sims = 0
        self.pending = False


class KeyedPool:
    """A caller's evaluated-tree pool.  reopen() starts a keyed session, open() an un-keyed one; both end the last session.  The
    host's rule: `played` reaches the rows only if the last session was keyed, has no wave waiting for its backup, and had this call's
    shape (rows, lo, node_cap, k_cap, legal_words, n_par)."""

    def __init__(self):
        self.rows, self.shape, self.keyed, self.session = [], None, False, None

    def invalidate(self):
        """xr_batch_set_groups (xr_batch_load_regions drops the pool altogether)."""
        self.keyed = False

    def open(self, legal_rows, n_par, node_cap, E, max_sims, k_cap, priors=None):
        self.keyed = False
        self.session = et.Session(legal_rows, n_par, node_cap, E, max_sims, k_cap, priors)
        return self.session

    def reopen(self, states, played, n_par, node_cap, E, max_sims, k_cap, priors=None, lo=0, legal_words=1):
        """(the Session, kept [rows][2])."""
        if not 1 <= n_par <= max_sims <= MAX_SIMS:
            raise ValueError("max_sims outside n_par .. XR_TREE_MAX_SIMS")
        shape = (len(states), lo, node_cap, k_cap, legal_words, n_par)
        pending = self.session is not None and self.session.pending
        if not self.keyed or pending or shape != self.shape:
            self.rows, played = [KeyedRow() for _ in states], None
        self.shape, self.keyed = shape, True
        trees, kept = [], []
        for r, st in enumerate(states):
            t, k = self.rows[r].begin(st, None if played is None else int(played[r]), max_sims, node_cap, E, None if priors is None else priors[r])
            trees.append(t)
            kept.append(k)
        self.session = Session(trees, n_par, max_sims, k_cap)
        return self.session, kept
