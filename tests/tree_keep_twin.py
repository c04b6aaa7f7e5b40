"""XR-Tree v1, kept (include/xroute_hip.h, "---- kept trees") as plain Python over tests/tree_twin.RowTree: the key check, the
re-rooting with the spec's operation order (W' = W - float(N) * r: one multiplication, then one subtraction), the row-state shift and
the long exploration table.  The twin of xr_batch_tree_search_keep for the tests: the returns come from a callable, as in tree_twin.
A KeptRow is one row of a caller's kept-tree pool; a KeptPool is the caller's pool (the host's shape check included)."""
import copy

from tests import tree_twin
from tests.tree_twin import INF, RowTree

KEPT = 2
MAX_SIMS = 65536


class State:
    """What the key holds of an env: env_steps, region, replay, the legal nets (1-based); reward: the slot's reward row."""

    def __init__(self, env_steps, region, replay, legal, reward=0.0):
        self.env_steps = int(env_steps)
        self.region = int(region)
        self.replay = int(replay)
        self.legal = sorted(int(n) for n in legal)
        self.reward = float(reward)


def shifted(node, r):
    nd = copy.copy(node)
    nr = float(nd.N) * r
    nd.W = nd.W - nr
    nd.V = 0
    return nd


class KeptRow:
    def __init__(self):
        self.tree = None
        self.key = None          # a State, or None: not valid

    def _mode(self, st, played, n_add):
        """(0 rebuild | 1 whole | 2 re-root, index of the played child)."""
        k, t = self.key, self.tree
        if not st.legal or played is None or played < 0 or k is None or t is None:
            return 0, -1
        if k.region != st.region or k.replay != st.replay:
            return 0, -1
        if played == 0:
            if k.env_steps != st.env_steps or k.legal != st.legal or not t.nodes or t.nodes[0].N + n_add > MAX_SIMS:
                return 0, -1
            return 1, -1
        if k.env_steps + 1 != st.env_steps or played not in k.legal or [n for n in k.legal if n != played] != st.legal:
            return 0, -1
        if not t.nodes or t.nodes[0].first < 0:
            return 0, -1
        root = t.nodes[0]
        for i in range(root.first, root.first + root.count):
            if t.nodes[i].net == played:
                return (2, i) if t.nodes[i].N + n_add <= MAX_SIMS else (0, -1)
        return 0, -1

    def begin(self, st, played, n_add, node_cap, E, prior=None):
        """The call's first kernel for this row: returns (the RowTree the call searches in, kept = [N of the new root, nodes carried])."""
        mode, child = self._mode(st, played, n_add)
        old = self.tree
        tree = RowTree(st.legal, node_cap, E, prior)          # mode 0: exactly this
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


class KeptPool:
    """A caller's pool: rows of KeptRow, rebuilt as a whole when the call's shape differs from the last call's."""

    def __init__(self):
        self.rows, self.shape = [], None

    def search(self, states, played, n_waves, n_par, node_cap, E, evaluate, k_cap, priors=None, lo=0):
        """tree_twin.search for a kept call.  states: a State per row; played: None or a list per row.  Returns (results per row with
        "kept" added, paths, returns, the RowTree objects)."""
        shape = (len(states), lo, node_cap, k_cap)
        if shape != self.shape:
            self.rows, self.shape, played = [KeptRow() for _ in states], shape, None
        trees, kept = [], []
        for r, st in enumerate(states):
            t, k = self.rows[r].begin(st, None if played is None else int(played[r]), n_waves * n_par, node_cap, E,
                                      None if priors is None else priors[r])
            trees.append(t)
            kept.append(k)
        all_paths = [[] for _ in trees]
        all_returns = [[] for _ in trees]
        for w in range(n_waves):
            paths = [t.select(n_par) for t in trees]
            returns, orders = evaluate(w, paths)
            for r, t in enumerate(trees):
                t.backup(returns[r], orders[r])
                all_paths[r] += [(list(p) + [0] * k_cap)[:k_cap] for p in paths[r]]
                all_returns[r] += [float(g) for g in returns[r]]
        results = []
        for t, k in zip(trees, kept):
            res = t.result(k_cap)
            res["kept"] = k
            results.append(res)
        return results, all_paths, all_returns, trees


assert tree_twin.POOL_FULL == 1 and INF == float("inf")
