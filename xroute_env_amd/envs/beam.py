"""Beam search over net orderings, composed on the host from device tensors: lookahead -> select -> branch -> step.

The batch holds len(regions) * width slots; slots [r * W, (r + 1) * W) are the beams of region r.  At every ply `lookahead` prices every
net every beam may still pick, the W best (beam, net) pairs of a region survive, `branch` makes slot j of the region continue from the
state of the pair's beam and a route-only `step` routes the pair's net.  The selection is policy, not hot path: a stable sort of a
[regions, W * k_max] table per ply.  The chosen net is routed twice, once priced (lookahead) and once stepped; the step's reward must
carry the bits lookahead promised.
"""
from __future__ import annotations

import time
from typing import List, Optional, Sequence

import torch

from ..batch import RegionBatch

NEG_INF = float("-inf")


def select_beams(value: torch.Tensor, width: int):
    """The W best (parent, net) pairs of every region.  value: float64 [regions, W, k_max] — the return a region's beam `parent` would
    have after routing net `net + 1`; -inf: not a candidate (a dead beam's whole row).  Order: value descending, then parent ascending,
    then net ascending (a stable sort over the flat (parent, net) index, not topk: equal inputs give equal orders).  Returns
    (parent int64 [regions, width], net int64 [regions, width] 1-based, alive bool [regions, width]); where fewer than `width` finite
    candidates exist the rest are dead beams: parent -1, net 0."""
    if value.dim() != 3:
        raise ValueError("value must be [regions, beams, nets]")
    R, W, K = value.shape
    width = int(width)
    if width < 1:
        raise ValueError(f"width must be >= 1, got {width}")
    flat = value.reshape(R, W * K)
    val, idx = torch.sort(flat, dim=1, descending=True, stable=True)
    if W * K < width:                      # fewer pairs than beams: the missing ones are dead
        pad = width - W * K
        val = torch.cat([val, torch.full((R, pad), NEG_INF, dtype=val.dtype, device=val.device)], dim=1)
        idx = torch.cat([idx, torch.zeros((R, pad), dtype=idx.dtype, device=idx.device)], dim=1)
    val, idx = val[:, :width], idx[:, :width]
    alive = val > NEG_INF
    parent = torch.where(alive, idx // K, torch.full_like(idx, -1))
    net = torch.where(alive, idx % K + 1, torch.zeros_like(idx))
    return parent, net, alive


def beam_search(regions: Sequence, width: int, device="cuda:0", stats: Optional[dict] = None, **batch_kw) -> List[List[dict]]:
    """Beam search of width `width` over the net orderings of every region, all regions at once.  Returns, per region, its beams best
    first (return descending, ties in slot order), each {"order": [net ids], "ret": float (the rewards summed in step order in double),
    "delta": [violation, wirelength, via] summed, "status": OR of the steps' status bits}.  Only beams that are alive at the end are
    reported (at least one per region).  batch_kw goes to RegionBatch (router knobs, costs); auto_reset is off.  stats: an optional dict
    that receives "ply_ms", the host time of every ply (each ply ends in a host read of the selection, so this is wall time)."""
    W, R = int(width), len(regions)
    if W < 1 or R < 1:
        raise ValueError("beam_search needs width >= 1 and at least one region")
    batch_kw.pop("auto_reset", None)
    b = RegionBatch(regions, n_envs=R * W, device=device, auto_reset=False, **batch_kw)
    try:
        return _search(b, R, W, stats)
    finally:
        b.close()


def _search(b: RegionBatch, R: int, W: int, stats: Optional[dict] = None) -> List[List[dict]]:
    dev, K = b.device, max(int(b.k_max), 1)
    b.assign([r for r in range(R) for _ in range(W)])
    b.reset()
    alive = torch.zeros((R, W), dtype=torch.bool, device=dev)
    alive[:, 0] = True                                                   # ply 0: one beam per region
    ret = torch.zeros((R, W), dtype=torch.float64, device=dev)
    delta = torch.zeros((R, W, 3), dtype=torch.int64, device=dev)
    status = torch.zeros((R, W), dtype=torch.int32, device=dev)
    order = torch.zeros((R, W, K), dtype=torch.int32, device=dev)
    base = (torch.arange(R, device=dev) * W).unsqueeze(1)               # first slot of every region
    neg = torch.full((R, W, K), NEG_INF, dtype=torch.float64, device=dev)
    from ..dist import unpack_records
    ply_ms = []
    for ply in range(K + 1):
        t0 = time.perf_counter()
        _, reward = b.lookahead()
        value = torch.where(alive.unsqueeze(2), ret.unsqueeze(2) + reward.view(R, W, K), neg)
        parent, net, now = select_beams(value, W)
        if not bool(now.any()):                                          # no candidate left anywhere
            break
        if ply >= K:
            raise RuntimeError("beam_search: candidates left after k_max plies")
        # a region without a candidate has finished (its beams all routed their last net at the same ply): its beams stay as they are
        open_ = now.any(dim=1, keepdim=True)
        src = torch.where(now, parent, torch.arange(W, device=dev).expand(R, W))      # (a beam that does not move keeps its own row)
        b.branch(torch.where(now, parent + base, torch.full_like(parent, -1)).reshape(-1).to(torch.int32).contiguous())
        idx = src.unsqueeze(2)
        order = order.gather(1, idx.expand(R, W, K)).clone()
        delta = delta.gather(1, idx.expand(R, W, 3))
        ret, status = ret.gather(1, src), status.gather(1, src)
        promised = value.reshape(R, W * K).gather(1, (src * K + (net - 1).clamp(min=0)))
        b.step(net.reshape(-1).to(torch.int32).contiguous())            # route only
        rec = unpack_records(b.fetch("record"))
        ret = torch.where(now, ret + rec["reward"].view(R, W), ret)
        if not torch.equal(ret[now], promised[now]):
            raise RuntimeError("beam_search: a step's reward differs from what lookahead promised for that (state, net)")
        delta = torch.where(now.unsqueeze(2), delta + rec["delta"].view(R, W, 3).to(torch.int64), delta)
        status = torch.where(now, status | rec["status"].view(R, W).to(torch.int32), status)
        order[:, :, ply] = torch.where(now, net.to(torch.int32), torch.zeros_like(order[:, :, ply]))
        alive = torch.where(open_, now, alive)
        ply_ms.append((time.perf_counter() - t0) * 1e3)
    if stats is not None:
        stats["ply_ms"] = ply_ms
    rank = torch.sort(torch.where(alive, ret, torch.full_like(ret, NEG_INF)), dim=1, descending=True, stable=True).indices.cpu()
    alive_h, ret_h, delta_h, status_h, order_h = alive.cpu(), ret.cpu(), delta.cpu(), status.cpu(), order.cpu()
    out = []
    for r in range(R):
        beams = []
        for j in rank[r].tolist():
            if not alive_h[r, j]:
                continue
            beams.append({"order": [int(v) for v in order_h[r, j].tolist() if v > 0], "ret": float(ret_h[r, j]),
                          "delta": [int(v) for v in delta_h[r, j].tolist()], "status": int(status_h[r, j])})
        out.append(beams)
    return out
