"""Tree search episodes: search, step the chosen net, repeat — the play loop of the reference's MCTS agent
(baseline/xroute/self_route.py:341-371) with the whole search on the device (RegionBatch.tree_search, XR-Tree v1).

One slot per region.  At every ply one enqueue-only tree search per env prices the env's next net: the most visited child of the root
(ties to the higher value, then to the lower net) is stepped.  The tree is rebuilt at every ply (no reuse between calls) unless
reuse=True: then the search of a ply continues from the subtree below the net just stepped ("XR-Tree v1, kept").  Every
simulation is a complete ordering of the env's remaining nets, so besides the order it played a region also reports the best ordering
any simulation saw: the nets already played followed by the best line of the search that saw it.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence

import torch

from ..batch import RegionBatch
from .vector_env import XRouteVectorEnv


def lookahead_prior(batch: RegionBatch, temperature: float) -> torch.Tensor:
    """float32 [n_envs, k_max]: softmax over every env's legal nets of its lookahead rewards divided by `temperature` (the maximum
    subtracted first); 0 for a net that is not a candidate."""
    if not temperature > 0:
        raise ValueError(f"temperature must be > 0, got {temperature}")
    _, reward = batch.lookahead()
    top = reward.max(dim=1, keepdim=True).values
    top = torch.where(torch.isfinite(top), top, torch.zeros_like(top))
    return torch.exp((reward - top) / float(temperature)).to(torch.float32).contiguous()          # (exp(-inf) == 0: not a candidate)


def tree_episodes(regions: Sequence, n_waves: int, n_par: int, seed: int = 0, device="cuda:0", prior: Optional[Callable] = None,
                  node_cap: Optional[int] = None, c_init: float = 1.25, c_base: float = 19652.0, stats: Optional[dict] = None,
                  sim_weights: Optional[Callable] = None, reuse: bool = False, waves_after: Optional[int] = None, **batch_kw) -> List[dict]:
    """Play every region's episode by tree search, all regions at once.  Returns per region {"order": the nets played, "ret": the
    episode's return (the step rewards summed in step order in double), "best_order": the best complete ordering any simulation of any
    ply saw, "best_ret": its return, "simulations": the simulations run}.  prior: None, or a callable (batch) -> float32 [n_envs,
    k_max] weights asked before every search (lookahead_prior is one).  The seed of ply p is seed + p.  batch_kw goes to RegionBatch
    (router knobs, costs); auto_reset is off.  stats: an optional dict that receives "routed_nets", the nets the searches routed.
    sim_weights: None (random simulations), or a callable (batch) -> int32 [n_envs, k_max] weights asked before every search: the
    simulations follow the weighted policy (envs.weighted.lookahead_weights is one).  reuse: search, step, continue with the actions
    just stepped (RegionBatch.tree_search(keep=True, played=...)); stats then also receives "carried_visits" and "carried_nodes", the
    sums over plies and regions of what the kept trees brought along, and "plies", the searches of live envs.  waves_after: the waves of
    every ply but the first (default n_waves)."""
    R = len(regions)
    if R < 1:
        raise ValueError("tree_episodes needs at least one region")
    batch_kw.pop("auto_reset", None)
    b = RegionBatch(regions, n_envs=R, device=device, auto_reset=False, **batch_kw)
    try:
        b.reset()
        K = max(int(b.k_max), 1)
        dev = b.device
        ret = torch.zeros(R, dtype=torch.float64, device=dev)
        order = torch.zeros((R, K), dtype=torch.int32, device=dev)
        best_ret = torch.full((R,), float("-inf"), dtype=torch.float64, device=dev)
        best_order = torch.zeros((R, K), dtype=torch.int32, device=dev)
        sims = torch.zeros(R, dtype=torch.int64, device=dev)
        routed = 0
        if reuse and node_cap is None:          # one pool shape for every ply, with room for what the trees carry along
            node_cap = 1 + 4 * int(n_waves) * int(n_par) * K
        played, carried = None, torch.zeros(2, dtype=torch.int64, device=dev)
        live_plies = 0
        from ..dist import unpack_records
        for ply in range(K + 1):
            nl = b.fetch("nlegal")
            if not bool((nl > 0).any()):                     # (the one host read of a ply)
                break
            if ply >= K:
                raise RuntimeError("tree_episodes: nets left after k_max plies")
            waves = int(n_waves) if ply == 0 or waves_after is None else int(waves_after)
            res = b.tree_search(waves, n_par, seed + ply, prior(b) if prior is not None else None, node_cap, c_init, c_base,
                                sim_weights=sim_weights(b) if sim_weights is not None else None, keep=reuse, played=played)
            if reuse:
                carried += res["kept"].to(torch.int64).sum(dim=0)
            live_plies += int((nl > 0).sum())
            act = XRouteVectorEnv._most_visited(res)
            # the best line of this search, as a whole episode: what was played so far, then the line
            line = res["best_return"] + ret
            better = line > best_ret
            whole = order.clone()
            if ply < K:
                whole[:, ply:] = res["best_order"][:, :K - ply]
            best_order = torch.where(better.unsqueeze(1), whole, best_order)
            best_ret = torch.where(better, line, best_ret)
            sims += res["info"][:, 0].to(torch.int64)
            routed += waves * int(n_par) * int(nl.sum())          # every simulation of a live env routes all its remaining nets
            b.step(act)
            rec = unpack_records(b.fetch("record"))
            live = act > 0
            ret = torch.where(live, ret + rec["reward"], ret)
            order[:, ply] = act
            played = act if reuse else None
        if stats is not None:
            stats["routed_nets"] = routed
            stats["plies"] = live_plies
            if reuse:
                stats["carried_visits"], stats["carried_nodes"] = (int(v) for v in carried.cpu().tolist())
        ret_h, order_h, bret_h, border_h, sims_h = ret.cpu(), order.cpu(), best_ret.cpu(), best_order.cpu(), sims.cpu()
        return [{"order": [int(v) for v in order_h[r].tolist() if v > 0], "ret": float(ret_h[r]),
                 "best_order": [int(v) for v in border_h[r].tolist() if v > 0], "best_ret": float(bret_h[r]), "simulations": int(sims_h[r])}
                for r in range(R)]
    finally:
        b.close()
