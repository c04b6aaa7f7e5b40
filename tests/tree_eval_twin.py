""""XR-Tree v2, evaluated" (include/xroute_hip.h, "---- evaluated tree search") as plain Python: floats, one operation per line, no numpy in
the arithmetic.  The twin of xr_batch_tree_open / _leaves / _backup for the tests.  Nodes, Prior, Select's score and Backup's additions
are tests/tree_twin.py's (imported, not edited); what is new here is the leaf record of a selection, G = line return + value, the best
line from terminal simulations only, and the evaluator's prior over the children of a fresh leaf.  The line returns, the values and the
priors are arguments, so the same code runs on hand-made numbers without a GPU (tests/test_tree_eval_host.py) and on the device's own
peek returns beside the device session (tests/test_gpu_tree_eval.py)."""
import math

from tests import tree_twin

TERMINAL, FRESH, NONE = 1, 2, 4
INF = float("inf")


class EvalRowTree(tree_twin.RowTree):
    """One row of a session.  legal: the env's legal nets at the open call; prior: None or the open call's row prior."""

    def __init__(self, legal, node_cap, E, prior=None):
        super().__init__(legal, node_cap, E, prior)
        self.wave_leaves = []          # (node index, flags) of the current wave, per lane
        self.wave_nets = []            # and the nets of its paths
        self.repriored = 0             # blocks an evaluator's prior was written to (what the tests ask their inputs to show)

    def select(self, n_par):
        """One wave: (paths, leaf records) of lanes 0 .. n_par - 1."""
        if self.done:
            self.wave_leaves = [(-1, NONE)] * n_par
            return [[] for _ in range(n_par)], list(self.wave_leaves)
        paths = []
        self.wave_paths, self.wave_leaves, self.wave_nets = [], [], []
        for _ in range(n_par):
            node, idx, nets = 0, [0], []
            while self.nodes[node].first >= 0:
                node = self._best_child(self.nodes[node])
                idx.append(node)
                nets.append(self.nodes[node].net)
            flags = 0
            if len(nets) >= len(self.legal):
                flags = TERMINAL
                self.terminal_visits += 1
            else:
                self._expand(node, nets)
                if self.nodes[node].first >= 0:
                    flags = FRESH
            for i in idx:
                self.nodes[i].V += 1
            self.max_depth = max(self.max_depth, len(nets))
            self.wave_paths.append(idx)
            self.wave_leaves.append((node, flags))
            self.wave_nets.append(list(nets))
            paths.append(nets)
        return paths, list(self.wave_leaves)

    def backup(self, line_returns, values, leaf_priors=None):
        """The wave's line returns and values in lane order (and None, or one prior row per lane).  Returns the wave's G."""
        if self.done:
            return [0.0] * len(line_returns)
        out = []
        for j, (idx, (leaf, flags), nets) in enumerate(zip(self.wave_paths, self.wave_leaves, self.wave_nets)):
            G = float(line_returns[j])
            if not flags & TERMINAL:
                v = float(values[j])
                if not math.isfinite(v):
                    v = 0.0
                G = G + v
            for i in idx:
                nd = self.nodes[i]
                nd.N += 1
                nd.V -= 1
                nd.W = nd.W + G
            self.mn = min(self.mn, G)
            self.mx = max(self.mx, G)
            if flags & TERMINAL and G > self.best:
                self.best = G
                self.best_order = list(nets)
            self.sims += 1
            out.append(G)
            if leaf_priors is not None and flags & FRESH:
                w = leaf_priors[j]
                nd = self.nodes[leaf]
                S = 0.0
                for i in range(nd.first, nd.first + nd.count):
                    S = S + tree_twin.weight(w[self.nodes[i].net - 1])
                if S > 0.0:
                    for i in range(nd.first, nd.first + nd.count):
                        self.nodes[i].P = tree_twin.weight(w[self.nodes[i].net - 1]) / S
                    self.repriored += 1
        return out


class Session:
    """xr_batch_tree_open for a list of rows, then leaves() / backup() in turn.  The call-order rules are the library's."""

    def __init__(self, legal_rows, n_par, node_cap, E, max_sims, k_cap, priors=None):
        if not 1 <= n_par <= max_sims:
            raise ValueError("max_sims below n_par")
        self.trees = [EvalRowTree(legal, node_cap, E, None if priors is None else priors[r]) for r, legal in enumerate(legal_rows)]
        self.n_par, self.max_sims, self.k_cap = n_par, max_sims, k_cap
        self.sims = 0
        self.pending = False

    def leaves(self):
        """(paths [rows][n_par][k_cap] zero-padded, leaf records [rows][n_par][2])."""
        if self.pending:
            raise RuntimeError("leaves twice without a backup")
        if self.sims + self.n_par > self.max_sims:
            raise OverflowError("the wave would pass max_sims")
        paths, leaves = [], []
        for t in self.trees:
            p, l = t.select(self.n_par)
            paths.append([(list(x) + [0] * self.k_cap)[:self.k_cap] for x in p])
            leaves.append([list(x) for x in l])
        self.pending = True
        return paths, leaves

    def backup(self, line_returns, values, leaf_priors=None):
        """Returns (results per row as tree_twin's result(), the wave's G [rows][n_par])."""
        if not self.pending:
            raise RuntimeError("backup without pending leaves")
        G = [t.backup(line_returns[r], values[r], None if leaf_priors is None else leaf_priors[r]) for r, t in enumerate(self.trees)]
        self.pending = False
        self.sims += self.n_par
        return [t.result(self.k_cap) for t in self.trees], G
