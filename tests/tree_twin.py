"""XR-Tree v1 (include/xroute_hip.h, "---- tree search") as plain Python: floats, one operation per line, no numpy in the arithmetic.  The
twin of xr_batch_tree_search for the tests: the returns of the simulations come from a callable, so the same code runs on hand-made
returns without a GPU (tests/test_tree_host.py) and on RegionBatch.rollout's returns beside the device search (tests/test_gpu_tree.py).
The exploration table is an argument: the tests take it from xr_tree_exploration_table, so nothing rests on two math libraries agreeing."""
import math

POOL_FULL = 1
INF = float("inf")


def weight(x):
    """A prior entry: not finite or < 0 counts as 0."""
    x = float(x)
    if math.isfinite(x) and x >= 0.0:
        return x
    return 0.0


class Node:
    __slots__ = ("N", "V", "W", "P", "net", "first", "count")

    def __init__(self, net, P):
        self.N = 0
        self.V = 0
        self.W = 0.0
        self.P = P
        self.net = net
        self.first = -1
        self.count = 0


class RowTree:
    """The tree of one row.  legal: the env's legal nets (1-based); prior: None or a sequence indexed by net - 1."""

    def __init__(self, legal, node_cap, E, prior=None):
        self.legal = sorted(int(n) for n in legal)
        self.node_cap = int(node_cap)
        self.E = E
        self.prior = prior
        self.mn = INF
        self.mx = -INF
        self.best = -INF
        self.best_order = None
        self.flags = 0
        self.max_depth = 0
        self.sims = 0
        self.nodes = []
        self.wave_paths = []          # node indices of the current wave's paths, per lane
        # what the tests ask their inputs to show
        self.ties = 0                 # selections whose maximum two or more children shared
        self.terminal_visits = 0      # paths that ended at a terminal node
        self.done = not self.legal
        if not self.done:
            self.nodes.append(Node(0, 1.0))
            self._expand(0, [])

    def _expand(self, node, path_nets):
        nets = [n for n in self.legal if n not in path_nets]
        cnt = len(nets)
        first = len(self.nodes)
        if cnt > self.node_cap - first:
            self.flags |= POOL_FULL
            return
        S = 0.0
        if self.prior is not None:
            for n in nets:
                S = S + weight(self.prior[n - 1])
        uniform = self.prior is None or not (S > 0.0)
        pu = 1.0 / float(cnt)
        for n in nets:
            self.nodes.append(Node(n, pu if uniform else weight(self.prior[n - 1]) / S))
        self.nodes[node].first = first
        self.nodes[node].count = cnt

    def _best_child(self, p):
        n_p = p.N + p.V
        Ep = self.E[n_p]
        best_i, best_s, shared = -1, 0.0, 1
        for i in range(p.first, p.first + p.count):
            c = self.nodes[i]
            n_c = c.N + c.V
            u = Ep * c.P
            u = u / float(n_c + 1)
            v = 0.0
            if c.N > 0 and self.mx > self.mn:
                v = c.W / float(c.N)
                v = v - self.mn
                v = v / (self.mx - self.mn)
            s = u + v
            if best_i < 0 or s > best_s:
                best_i, best_s, shared = i, s, 1
            elif s == best_s:
                shared += 1
        if shared > 1:
            self.ties += 1
        return best_i

    def select(self, n_par):
        """One wave: the paths (lists of nets) of lanes 0 .. n_par - 1."""
        if self.done:
            return [[] for _ in range(n_par)]
        paths = []
        self.wave_paths = []
        for _ in range(n_par):
            node, idx, nets = 0, [0], []
            while self.nodes[node].first >= 0:
                node = self._best_child(self.nodes[node])
                idx.append(node)
                nets.append(self.nodes[node].net)
            if len(nets) < len(self.legal):
                self._expand(node, nets)
            else:
                self.terminal_visits += 1
            for i in idx:
                self.nodes[i].V += 1
            self.max_depth = max(self.max_depth, len(nets))
            self.wave_paths.append(idx)
            paths.append(nets)
        return paths

    def backup(self, returns, orders):
        """The wave's returns G and complete orderings, in lane order."""
        if self.done:
            return
        for idx, G, order in zip(self.wave_paths, returns, orders):
            G = float(G)
            for i in idx:
                nd = self.nodes[i]
                nd.N += 1
                nd.V -= 1
                nd.W = nd.W + G
            self.mn = min(self.mn, G)
            self.mx = max(self.mx, G)
            if G > self.best:
                self.best = G
                self.best_order = list(order)
            self.sims += 1

    def result(self, k_cap):
        visits = [0] * k_cap
        value = [-INF] * k_cap
        if self.done:
            return dict(visits=visits, value=value, info=[0, 0, 0, 0], best_order=[0] * k_cap, best_return=-INF)
        root = self.nodes[0]
        for i in range(root.first, root.first + root.count) if root.first >= 0 else ():
            c = self.nodes[i]
            visits[c.net - 1] = c.N
            if c.N > 0:
                value[c.net - 1] = c.W / float(c.N)
        order = list(self.best_order or [])
        order = (order + [0] * k_cap)[:k_cap]
        return dict(visits=visits, value=value, info=[self.sims, len(self.nodes), self.max_depth, self.flags], best_order=order, best_return=self.best)


def search(legal_rows, n_waves, n_par, node_cap, E, evaluate, k_cap, priors=None):
    """The whole call for a list of rows.  evaluate(w, paths) -> (returns [rows][n_par], orders [rows][n_par][<= k_cap]) with paths
    [rows][n_par] lists of nets: simulation (w, j) of every row.  Returns (results per row, paths [rows][n_waves * n_par] zero-padded to
    k_cap, returns [rows][n_waves * n_par], the RowTree objects)."""
    trees = [RowTree(legal, node_cap, E, None if priors is None else priors[r]) for r, legal in enumerate(legal_rows)]
    all_paths = [[] for _ in trees]
    all_returns = [[] for _ in trees]
    for w in range(n_waves):
        paths = [t.select(n_par) for t in trees]
        returns, orders = evaluate(w, paths)
        for r, t in enumerate(trees):
            t.backup(returns[r], orders[r])
            all_paths[r] += [(list(p) + [0] * k_cap)[:k_cap] for p in paths[r]]
            all_returns[r] += [float(g) for g in returns[r]]
    return [t.result(k_cap) for t in trees], all_paths, all_returns, trees
