"""Evaluated tree search: pUCT whose leaves a network values (RegionBatch.tree_open / tree_leaves / tree_backup, "XR-Tree v2,
evaluated" of include/xroute_hip.h) — the search of the reference's MuZero agent (baseline/xroute/self_route.py:341-371, 482-568) with
the tree, the routing and the network all on the device.

`evaluated_search` is the loop: open, then per wave leaves -> evaluate -> backup, all enqueued on one stream without a host
synchronisation.  An evaluator is a callable `evaluate(batch, leaves, group=None, stream=None) -> (value float64 [rows, n_par],
leaf_prior float32 [rows, n_par, k_max] or None)`; `leaves` is tree_leaves()'s dict (the packed state row of every leaf, the line
returns, the paths, the leaf records).  `critic_evaluator` values a leaf by an ActorCritic's critic over the obstacle tower of the
leaf's state; `actor_critic_evaluator` adds the softmax of the actor's logits over the leaf's legal nets as the prior of its children.
`evaluated_episodes` plays whole episodes with it, as envs.tree.tree_episodes does with the rollout search.  With keep / reuse the
sessions are "XR-Tree v2, kept" (RegionBatch.tree_open(keep=True, played=...)): a ply's session continues from the subtree below the net
just stepped.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence

import torch

from ..batch import RegionBatch
from .peek import _by_net, shape_groups, state_values
from .vector_env import XRouteVectorEnv


def evaluated_search(batch: RegionBatch, evaluate: Callable, n_waves: int, n_par: int, root_prior: Optional[torch.Tensor] = None,
                     node_cap: Optional[int] = None, c_init: float = 1.25, c_base: float = 19652.0, group: Optional[int] = None, stream=None,
                     trace: bool = False, keep: bool = False, played: Optional[torch.Tensor] = None):
    """n_waves waves of n_par evaluated simulations per row from the state every env is in now; the batch is left exactly as it was.
    keep=True: the kept session (RegionBatch.tree_open(keep=True, played=...), "XR-Tree v2, kept"): it continues from the tree the
    caller's last kept session left where `played` says how the envs have moved since, and the dict gains `kept` int32 [rows, 2] =
    {visits of the new root carried in, nodes carried}.
    Returns tree_backup()'s dict after the last wave {visits, value, info, best_order, best_return, returns}; with trace=True `paths`
    int32 [rows, n_waves * n_par, k_max], `returns` float64 [rows, n_waves * n_par] and `leaf` int32 [rows, n_waves * n_par, 2] hold
    every simulation in (wave, lane) order.  Nothing here reads a device value on the host: whether the loop synchronises is up to
    `evaluate`.  group: an env group (rows = its slots, enqueued on `stream`, default the current stream); None: the whole batch."""
    W, P = int(n_waves), int(n_par)
    if W < 1:
        raise ValueError(f"n_waves must be >= 1, got {n_waves}")
    if not callable(evaluate):
        raise ValueError("evaluate must be a callable (batch, leaves, group=, stream=) -> (value, leaf_prior or None)")
    if played is not None and not keep:
        raise ValueError("played needs keep=True")
    if keep:
        carried = batch.tree_open(P, W * P, root_prior, node_cap, c_init, c_base, group=group, stream=stream, keep=True, played=played)
    else:
        batch.tree_open(P, W * P, root_prior, node_cap, c_init, c_base, group=group, stream=stream)
    res, kept = None, {"paths": [], "returns": [], "leaf": []}
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(batch.device)):
        for _ in range(W):
            leaves = batch.tree_leaves(group=group, stream=stream)
            value, leaf_prior = evaluate(batch, leaves, group=group, stream=stream)
            res = batch.tree_backup(value, leaf_prior, group=group, stream=stream)
            if trace:
                kept["paths"].append(leaves["paths"]); kept["returns"].append(res["returns"]); kept["leaf"].append(leaves["leaf"])
        if trace:
            res = dict(res, **{k: torch.cat(v, dim=1) for k, v in kept.items()})
    if keep:
        res = dict(res, kept=carried)
    return res


def _leaf_pieces(batch, leaves, groups, group, stream):
    """The leaves' packed rows expanded shape by shape: yields (shape index, dims, rows_idx int64 [m] or None for every row, head fp32
    [m * n_par, 2 * n_max], nlegal, region int32 [m * n_par])."""
    rows, P, rb = leaves["rows"].shape
    for gi, (dims, idx) in enumerate(groups if groups is not None else shape_groups(batch, group, stream)):
        packed = leaves["rows"] if idx is None else leaves["rows"].index_select(0, idx)
        m = int(packed.shape[0])
        if m == 0:
            continue
        head, nlegal, region = batch.expand_state(packed.reshape(m * P, rb))
        yield gi, dims, idx, head, nlegal, region


def critic_evaluator(model, ob_towers=None, groups=None) -> Callable:
    """An evaluator for evaluated_search: value = model.critic(obstacle tower(leaf state)) in float64, no leaf prior.  Per shape group
    of the batch it runs expand_state on the leaves' packed rows, then peek.state_values.  model: an ActorCritic; ob_towers: a
    FusedObstacleTower or a dict {(X, Y, Z): FusedObstacleTower}, taken where ppo_actions would take it; groups: peek.shape_groups(batch)
    (computed per call when None: one host read for a batch of several grid shapes)."""
    @torch.no_grad()
    def evaluate(batch, leaves, group=None, stream=None):
        rows, P, _ = leaves["rows"].shape
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(batch.device)):
            value = torch.zeros((rows, P), dtype=torch.float64, device=batch.device)
            for _, dims, idx, head, _, _ in _leaf_pieces(batch, leaves, groups, group, stream):
                v = state_values(model, head, dims, ob_towers).to(torch.float64).reshape(-1, P)
                if idx is None:
                    value = v.contiguous()
                else:
                    value.index_copy_(0, idx, v)
        return value, None
    return evaluate


def actor_critic_evaluator(model, policy=None, groups=None) -> Callable:
    """An evaluator for evaluated_search: the critic's value as critic_evaluator gives it, and as leaf prior the softmax of the actor's
    logits over the leaf's legal nets (float32 [rows, n_par, k_max] by net: they sum to 1 over the legal nets of the leaf's state and
    are 0 elsewhere; all 0 for a terminal leaf).  policy: a GroupedFusedPolicy of (model, the batch) — built at the first call when
    None (it prefills the net-vector cache: host work, once per batch) — whose fused obstacle towers and fused actor head are taken
    where ppo_actions would take them, the module otherwise.  groups: peek.shape_groups(batch)."""
    from ..agents import GroupedFusedPolicy
    made = {}

    @torch.no_grad()
    def evaluate(b, leaves, group=None, stream=None):
        pol = policy
        if pol is None:
            if made.get("batch") is not b:
                made["batch"], made["policy"] = b, GroupedFusedPolicy(model, b)
            pol = made["policy"]
        rows, P, _ = leaves["rows"].shape
        k = max(int(b.k_max), 1)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(b.device)):
            value = torch.zeros((rows, P), dtype=torch.float64, device=b.device)
            prior = torch.zeros((rows, P, k), dtype=torch.float32, device=b.device)
            for _, dims, idx, head, nlegal, region in _leaf_pieces(b, leaves, groups, group, stream):
                g = pol.shapes.index(tuple(int(v) for v in dims))
                logits, nets, v = pol.group_logits(g, head, nlegal, region)
                lg = logits.to(torch.float64)
                top = lg.max(dim=1, keepdim=True).values
                top = torch.where(torch.isfinite(top), top, torch.zeros_like(top))
                e = torch.exp(lg - top)                                             # (exp(-inf) == 0: past the leaf's legal nets)
                p = (e / e.sum(dim=1, keepdim=True).clamp_min(1e-300)).to(torch.float32)
                p = _by_net(p, nets, 0.0).reshape(-1, P, k)
                v = v.to(torch.float64).reshape(-1, P)
                if idx is None:
                    value, prior = v.contiguous(), p.contiguous()
                else:
                    value.index_copy_(0, idx, v)
                    prior.index_copy_(0, idx, p)
        return value, prior
    return evaluate


def evaluated_episodes(regions: Sequence, evaluate, n_waves: int, n_par: int, device="cuda:0", root_prior: Optional[Callable] = None,
                       node_cap: Optional[int] = None, c_init: float = 1.25, c_base: float = 19652.0, stats: Optional[dict] = None,
                       reuse: bool = False, waves_after: Optional[int] = None, **batch_kw) -> List[dict]:
    """Play every region's episode by evaluated tree search, all regions at once (one slot per region): at every ply one session of
    n_waves x n_par simulations per env, then the most visited child of the root is stepped (ties to the higher value, then to the lower
    net).  evaluate: an evaluator (critic_evaluator, actor_critic_evaluator, or any callable of their form).  Returns per region {"order": the nets played, "ret": the episode's return (the step rewards
    summed in step order in double), "best_order": the best complete ordering a terminal simulation of any ply saw (the order played
    where none did), "best_ret": its return, "simulations": the simulations run}.  root_prior: None, or a callable (batch) -> float32
    [n_envs, k_max] asked before every search.  stats: an optional dict that receives "routed_nets", the nets the simulations routed
    (the sum of their path lengths), and "plies".  reuse: search, step, reopen with the actions just stepped ("XR-Tree v2, kept"): the
    session of a ply continues from the subtree below the net the env has played; one node_cap serves every ply (default 1 + 4 *
    (n_waves * n_par + 1) * k_max), and stats also receives "carried_visits" and "carried_nodes", the sums over plies and regions of
    what the kept trees brought along.  waves_after: the waves of every ply but the first (default n_waves)."""
    R = len(regions)
    if R < 1:
        raise ValueError("evaluated_episodes needs at least one region")
    batch_kw.pop("auto_reset", None)
    b = RegionBatch(regions, n_envs=R, device=device, auto_reset=False, **batch_kw)
    try:
        b.reset()
        ev = evaluate
        K = max(int(b.k_max), 1)
        dev = b.device
        ret = torch.zeros(R, dtype=torch.float64, device=dev)
        order = torch.zeros((R, K), dtype=torch.int32, device=dev)
        best_ret = torch.full((R,), float("-inf"), dtype=torch.float64, device=dev)
        best_order = torch.zeros((R, K), dtype=torch.int32, device=dev)
        sims = torch.zeros(R, dtype=torch.int64, device=dev)
        routed = torch.zeros((), dtype=torch.int64, device=dev)
        live_plies = 0
        carried = torch.zeros(2, dtype=torch.int64, device=dev)
        played = None
        if reuse and node_cap is None:          # one pool shape for every ply, with room for what the trees carry along
            node_cap = 1 + 4 * (int(n_waves) * int(n_par) + 1) * K
        from ..dist import unpack_records
        for ply in range(K + 1):
            nl = b.fetch("nlegal")
            if not bool((nl > 0).any()):                     # (the one host read of a ply)
                break
            if ply >= K:
                raise RuntimeError("evaluated_episodes: nets left after k_max plies")
            waves = int(n_waves) if ply == 0 or waves_after is None else int(waves_after)
            res = evaluated_search(b, ev, waves, n_par, root_prior(b) if root_prior is not None else None, node_cap, c_init, c_base, trace=True,
                                   keep=reuse, played=played)
            if reuse:
                carried += res["kept"].to(torch.int64).sum(dim=0)
            live_plies += int((nl > 0).sum())
            act = XRouteVectorEnv._most_visited(res)
            line = res["best_return"] + ret
            better = line > best_ret
            whole = order.clone()
            whole[:, ply:] = res["best_order"][:, :K - ply]
            best_order = torch.where(better.unsqueeze(1), whole, best_order)
            best_ret = torch.where(better, line, best_ret)
            sims += res["info"][:, 0].to(torch.int64)
            routed += (res["paths"] > 0).sum()
            b.step(act)
            rec = unpack_records(b.fetch("record"))
            live = act > 0
            ret = torch.where(live, ret + rec["reward"], ret)
            order[:, ply] = act
            played = act if reuse else None
        played_better = ret > best_ret                       # (no terminal simulation, or none as good as the line played)
        best_order = torch.where(played_better.unsqueeze(1), order, best_order)
        best_ret = torch.where(played_better, ret, best_ret)
        if stats is not None:
            stats["routed_nets"] = int(routed)
            stats["plies"] = live_plies
            if reuse:
                stats["carried_visits"], stats["carried_nodes"] = (int(v) for v in carried.cpu().tolist())
        ret_h, order_h, bret_h, border_h, sims_h = ret.cpu(), order.cpu(), best_ret.cpu(), best_order.cpu(), sims.cpu()
        return [{"order": [int(v) for v in order_h[r].tolist() if v > 0], "ret": float(ret_h[r]),
                 "best_order": [int(v) for v in border_h[r].tolist() if v > 0], "best_ret": float(bret_h[r]), "simulations": int(sims_h[r])}
                for r in range(R)]
    finally:
        b.close()
