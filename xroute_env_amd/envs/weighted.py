"""Weights for the weighted net sampling of include/xroute_hip.h ("XR-Pick v1"), and a cross-entropy search built on it.

The library draws a legal net with probability proportional to an int32 weight per net (RegionBatch.weighted_actions, rollout(policy=
"weighted"), tree_search(sim_weights=...)).  This module turns floats into such weights — `quantise`, `weights_from_scores`,
`lookahead_weights` — and runs `cem_search`: weighted rollouts whose weights are refitted to the best orderings seen, all of it device
tensors and enqueue-only calls (nothing here synchronises with the host).
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib

WEIGHT_ONE = 1 << 20          # the weight of a row's largest entry: 16 x below XR_WEIGHT_MAX, so a weight is never clamped


def quantise(p: torch.Tensor) -> torch.Tensor:
    """Non-negative floats [..., k] -> int32 weights of the same shape, row by row (the last axis is a row).  A finite p > 0 becomes
    max(1, round(p / rowmax * 2^20)) (rowmax = the row's largest finite entry; round half to even, in float64), so the row maximum maps to
    2^20, the order of the entries is kept (ties may appear, inversions cannot), and no positive entry loses its chance.  Zero, negative
    and non-finite entries become 0: such a net is drawn only when every legal net of the row has weight 0."""
    x = p.to(torch.float64)
    ok = torch.isfinite(x) & (x > 0)
    x = torch.where(ok, x, torch.zeros_like(x))
    top = x.max(dim=-1, keepdim=True).values
    q = torch.round(x / torch.where(top > 0, top, torch.ones_like(top)) * float(WEIGHT_ONE)).clamp(1.0, float(WEIGHT_ONE))
    return torch.where(ok, q, torch.zeros_like(q)).to(torch.int32)


def weights_from_scores(scores: torch.Tensor, temperature: float = 1.0) -> torch.Tensor:
    """Scores [..., k] (logits, rewards: higher is better) -> int32 weights: a float64 softmax over the finite entries of every row at
    `temperature` (> 0), then `quantise`.  Entries that are not finite (-inf of a net that is no candidate, NaN) get weight 0; every finite
    entry gets at least 1, however far below the row's best it lies."""
    t = float(temperature)
    if not (t > 0.0 and t < float("inf")):
        raise ValueError(f"temperature must be finite and > 0, got {temperature}")
    s = scores.to(torch.float64)
    ok = torch.isfinite(s)
    low = torch.where(ok, s, torch.full_like(s, float("-inf")))
    top = low.max(dim=-1, keepdim=True).values
    top = torch.where(torch.isfinite(top), top, torch.zeros_like(top))          # (a row without a finite entry: all weights 0)
    z = torch.where(ok, (s - top) / t, torch.zeros_like(s))
    # (the softmax's denominator cancels in quantise's p / rowmax; the floor keeps an underflowed exp positive)
    return quantise(torch.where(ok, torch.exp(z).clamp_min(1e-300), torch.zeros_like(z)))


def lookahead_weights(batch, temperature: float = 0.25, group: Optional[int] = None, stream=None) -> torch.Tensor:
    """int32 [rows, k_max] weights from one lookahead of the batch's current state: every candidate net's one-step reward, divided by
    the spread of its row (max - min over the candidates, at least 1), through `weights_from_scores` at `temperature` — at the default
    0.25 the cheapest next route is e^4 = 55 times as likely as the dearest.  Nets that are no candidates get 0."""
    _, reward = batch.lookahead(group=group, stream=stream)
    ok = torch.isfinite(reward)
    hi = torch.where(ok, reward, torch.full_like(reward, float("-inf"))).max(dim=1, keepdim=True).values
    lo = torch.where(ok, reward, torch.full_like(reward, float("inf"))).min(dim=1, keepdim=True).values
    spread = torch.where(torch.isfinite(hi - lo), hi - lo, torch.ones_like(hi)).clamp_min(1.0)
    return weights_from_scores(reward / spread, temperature)


def _first_max(ret: torch.Tensor):
    """(value, index) of the first maximum of every row of ret [rows, R] (argmax does not promise the first one)."""
    best = ret.max(dim=1, keepdim=True).values
    R = ret.shape[1]
    idx = torch.arange(R, device=ret.device).expand_as(ret)
    first = torch.where(ret == best, idx, torch.full_like(idx, R)).min(dim=1).values
    return best.squeeze(1), first


def cem_search(batch, n_iters: int, n_rollouts: int, n_elite: int, seed: int = 0, smoothing: float = 0.7, tau: float = 0.25,
               group: Optional[int] = None, stream=None):
    """Cross-entropy search over complete net orderings from the state every env is in now; the batch is left exactly as it was.
    Per env and iteration i = 0 .. n_iters - 1:
      1. R = n_rollouts orderings are played by rollout(R, _lib.tree_seed(seed, i), policy="weighted", weights=w_i); w_0 is all ones, so
         iteration 0 is rollout(R, seed, policy="random") bit for bit.
      2. The best-ever return and its order are kept (a later rollout replaces them only with a strictly higher return; within an
         iteration the first maximum wins).
      3. The elite are the n_elite rollouts of the highest return, ties to the lower rollout index.
      4. Every net's score is its mean position in the elite orders (0 = routed first; a net that an order does not hold counts as
         position k_max), scaled by the env's number of legal nets: z = -mean_pos / max(1, nlegal - 1), in [-1, 0] for the legal nets.
      5. p_new = softmax(z / tau) over the nets; p_{i+1} = smoothing * p_new + (1 - smoothing) * p_i with p_i = w_i normalised to sum 1;
         w_{i+1} = quantise(p_{i+1}).  The constants: smoothing 0.7, tau 0.25 (an always-first net is e^4 = 55 times as likely as an
         always-last one before smoothing).
    Returns (best_order int32 [rows, k_max], best_return float64 [rows], history float64 [n_iters, rows] = the best-ever return after
    every iteration: it never decreases).  A done env holds the empty rollout: order all 0, return 0.0.  Everything is torch on the
    device and enqueue-only; group / stream as in RegionBatch.rollout."""
    I, R, E = int(n_iters), int(n_rollouts), int(n_elite)
    if I < 1:
        raise ValueError(f"n_iters must be >= 1, got {n_iters}")
    if not 1 <= R <= _lib.XR_ROLLOUT_MAX:
        raise ValueError(f"n_rollouts must be in 1..{_lib.XR_ROLLOUT_MAX}, got {n_rollouts}")
    if not 1 <= E <= R:
        raise ValueError(f"n_elite must be in 1..n_rollouts = {R}, got {n_elite}")
    a, t = float(smoothing), float(tau)
    if not 0.0 < a <= 1.0:
        raise ValueError(f"smoothing must be in (0, 1], got {smoothing}")
    if not (t > 0.0 and t < float("inf")):
        raise ValueError(f"tau must be finite and > 0, got {tau}")
    rows = batch.n_envs if group is None else batch.group_bounds(group)[1] - batch.group_bounds(group)[0]
    k = max(int(batch.k_max), 1)
    dev = batch.device
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
        nlegal = batch.fetch("nlegal") if group is None else batch.fetch_group("nlegal", group, stream=stream)
        span = (nlegal.to(torch.float64) - 1.0).clamp_min(1.0).unsqueeze(1)
        w = torch.ones((rows, k), dtype=torch.int32, device=dev)
        best_ret = torch.full((rows,), float("-inf"), dtype=torch.float64, device=dev)
        best_order = torch.zeros((rows, k), dtype=torch.int32, device=dev)
        history = torch.empty((I, rows), dtype=torch.float64, device=dev)
        pos_of = torch.arange(k, device=dev, dtype=torch.float64).expand(rows, E, k)
        for i in range(I):
            res = batch.rollout(R, _lib.tree_seed(seed, i), policy="weighted", weights=w, group=group, stream=stream)
            ret, order = res["ret"], res["order"]
            top, first = _first_max(ret)
            better = top > best_ret
            cand = order.gather(1, first.view(rows, 1, 1).expand(rows, 1, k)).squeeze(1)
            best_order = torch.where(better.unsqueeze(1), cand, best_order)
            best_ret = torch.where(better, top, best_ret)
            history[i] = best_ret
            if i == I - 1:
                break
            elite = torch.sort(ret, dim=1, descending=True, stable=True).indices[:, :E]                       # (stable: ties to the lower index)
            eo = order.gather(1, elite.unsqueeze(2).expand(rows, E, k)).to(torch.int64)                        # [rows, E, k] nets in order
            pos = torch.full((rows, E, k + 1), float(k), dtype=torch.float64, device=dev)
            pos.scatter_(2, torch.where(eo > 0, eo - 1, torch.full_like(eo, k)), pos_of)                       # (column k: the orders' zero tail)
            z = -pos[:, :, :k].mean(dim=1) / span
            p_new = torch.softmax(z / t, dim=1)
            p_old = w.to(torch.float64)
            p_old = p_old / p_old.sum(dim=1, keepdim=True).clamp_min(1.0)
            w = quantise(a * p_new + (1.0 - a) * p_old).contiguous()
    return best_order, best_ret, history
