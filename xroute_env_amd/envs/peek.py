"""Successor states and their values, built on RegionBatch.peek (xr_batch_peek): "what state would the env be in?".

`successor_prefix` lists every env's candidate nets as one-net lines, `successor_states` peeks them and expands the packed rows into the
head rows step_compact writes, `successor_values` runs the obstacle tower and the critic of an ActorCritic over every successor,
`value_actions` picks the net of the highest reward + value, and `value_prior` turns such scores into the prior and the simulation
weights tree_search takes.  All of it is device tensors and enqueue-only calls; the one host round trip is `shape_groups` of a batch
whose regions have several grid shapes, and its result can be kept and passed in.
"""
from __future__ import annotations

from typing import Iterator, Optional, Tuple

import torch

from .weighted import weights_from_scores

DEFAULT_CHUNK = 64          # rows (envs) per expand_state call: chunk * k_max head rows of 2 * n_max floats are alive at a time


def prefix_from_legal(legal: torch.Tensor, k_max: int) -> torch.Tensor:
    """Legal-net bitmasks (int64 / uint64 [rows, legal_words], bit n - 1 of the row = net n) -> int32 [rows, k_max, 1]: line c holds the
    row's c-th legal net in ascending order, 0 past the number of legal nets among nets 1 .. k_max.  Works on any device."""
    k = max(int(k_max), 1)
    rows, words = int(legal.shape[0]), int(legal.shape[1])
    w = legal.view(torch.int64) if legal.dtype != torch.int64 else legal
    shifts = torch.arange(64, device=legal.device, dtype=torch.int64)
    bits = ((w.unsqueeze(2) >> shifts) & 1).reshape(rows, words * 64)          # (an arithmetic shift: the sign's copies are masked off)
    if words * 64 < k:
        bits = torch.cat([bits, bits.new_zeros((rows, k - words * 64))], dim=1)
    bits = bits[:, :k]
    rank = torch.cumsum(bits, dim=1) - 1                                        # position of a legal net among the row's legal nets
    out = torch.zeros((rows, k + 1), dtype=torch.int32, device=legal.device)
    ids = torch.arange(1, k + 1, device=legal.device, dtype=torch.int32).expand(rows, k)
    out.scatter_(1, torch.where(bits > 0, rank, torch.full_like(rank, k)), ids)          # (column k: the bin of the nets that are not legal)
    return out[:, :k].unsqueeze(2).contiguous()


def successor_prefix(batch, group: Optional[int] = None, stream=None) -> torch.Tensor:
    """int32 [rows, k_max, 1] on the batch device: line c of an env holds its c-th legal net in ascending order, 0 past nlegal — the
    prefix under which peek / rollout(policy="stop") visit every one-net successor of every env."""
    legal = batch.fetch("legal") if group is None else batch.fetch_group("legal", group, stream=stream)
    return prefix_from_legal(legal, batch.k_max)


def shape_groups(batch, group: Optional[int] = None, stream=None):
    """The rows of the batch (or of one env group) by the grid shape of the region they play: a list of ((X, Y, Z), idx) with idx an
    int64 device tensor of row indices, or None for "every row" when all regions have one shape.  The towers take one grid shape per
    call, so successors are evaluated shape by shape.  With several shapes this reads the slots' regions back (ONE host round trip);
    the result stays valid for as long as the slots keep their regions, and every function below takes it as `groups=` — with it, or
    with regions of one shape, nothing here synchronises with the host."""
    shapes = sorted({tuple(int(v) for v in r.dims) for r in batch.regions})
    if len(shapes) == 1:
        return [(shapes[0], None)]
    region = batch.fetch("region") if group is None else batch.fetch_group("region", group, stream=stream)
    table = torch.tensor([shapes.index(tuple(int(v) for v in r.dims)) for r in batch.regions], dtype=torch.int64, device=region.device)
    sid = table[region.to(torch.int64)]
    return [(shape, (sid == g).nonzero()[:, 0]) for g, shape in enumerate(shapes)]


def successor_states(batch, group: Optional[int] = None, chunk: int = DEFAULT_CHUNK, stream=None, groups=None) -> Iterator[Tuple]:
    """Peek every one-net successor of every env (one launch), then expand the packed rows shape by shape, `chunk` envs at a time.
    Yields (dims (X, Y, Z), rows_idx int64 [m] — the envs of this piece —, head fp32 [m * k_max, 2 * n_max], nlegal int32 [m * k_max],
    region int32 [m * k_max], reward float64 [m, k_max], nets int32 [m, k_max]).  Head row j * k_max + c is what step_compact would
    write for env rows_idx[j] after its c-th legal net nets[j, c]; where nets is 0 (past the env's nlegal, a done env) the row is the
    env's CURRENT state and the reward 0.0.  reward is the successor's step reward (peek's `ret`).  groups: `shape_groups(batch)`."""
    if int(chunk) < 1:
        raise ValueError(f"chunk must be >= 1, got {chunk}")
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(batch.device)):
        prefix = successor_prefix(batch, group, stream)
        res = batch.peek(prefix, group=group, stream=stream)
        rows, k, rb = res["rows"].shape
        every = torch.arange(rows, device=batch.device)
        for dims, idx in (groups if groups is not None else shape_groups(batch, group, stream)):
            idx = every if idx is None else idx
            for lo in range(0, int(idx.numel()), int(chunk)):
                sel = idx[lo:lo + int(chunk)]
                m = int(sel.numel())
                head, nlegal, region = batch.expand_state(res["rows"].index_select(0, sel).reshape(m * k, rb))
                yield dims, sel, head, nlegal, region, res["ret"].index_select(0, sel), prefix[:, :, 0].index_select(0, sel)


def _fused_tower(ob_towers, dims_xyz):
    """The fused obstacle tower of a region shape where ppo_actions would take it: there, supported, eval mode, built for this shape."""
    X, Y, Z = dims_xyz
    t = ob_towers.get((X, Y, Z)) if isinstance(ob_towers, dict) else ob_towers
    return t if (t is not None and t.supported and not t.rep.training and t.dims == (Z, Y, X)) else None


@torch.no_grad()
def state_values(model, head: torch.Tensor, dims, ob_towers=None) -> torch.Tensor:
    """fp32 [n]: model.critic(state vector of head row i) for head rows of ONE grid shape dims = (X, Y, Z) in the step_compact /
    expand_state layout (plane 0 first).  ob_towers: a FusedObstacleTower or a dict {(X, Y, Z): FusedObstacleTower}; the fused tower
    is taken where ppo_actions would take it (supported, eval mode, built for this shape, contiguous rows), and
    normalize(encode_obstacles) of the module otherwise."""
    from ..agents import normalize
    X, Y, Z = (int(v) for v in dims)
    t = _fused_tower(ob_towers, (X, Y, Z)) if head.is_contiguous() else None
    if t is not None:
        state = t(head)
    else:
        state = normalize(model.representation_network.encode_obstacles(head[:, :X * Y * Z].reshape(head.shape[0], 1, Z, Y, X)))
    return model.critic(state)[:, 0]


def _by_net(x: torch.Tensor, nets: torch.Tensor, fill: float) -> torch.Tensor:
    """x [rows, k] indexed by candidate rank -> [rows, k] indexed by net (column n - 1 = net n = nets[row, rank]); `fill` elsewhere."""
    rows, k = nets.shape
    out = torch.full((rows, k + 1), fill, dtype=x.dtype, device=x.device)
    out.scatter_(1, torch.where(nets > 0, nets.to(torch.int64) - 1, torch.full(nets.shape, k, dtype=torch.int64, device=nets.device)), x)
    return out[:, :k].contiguous()          # (column k: the bin of the lines without a net)


@torch.no_grad()
def successor_values(model, batch, ob_towers=None, group: Optional[int] = None, chunk: int = DEFAULT_CHUNK, stream=None,
                     return_rewards: bool = False, groups=None):
    """fp32 [rows, k_max], indexed by net like lookahead's tables: column n - 1 holds critic(tower(head)) of the state the env is in
    after routing net n now, -inf where net n is no candidate (not legal, a done env).  model: an ActorCritic; ob_towers as
    `state_values` takes them; groups: `shape_groups(batch)` (computed here when None).  With return_rewards: (values, reward float64
    [rows, k_max]) — the successor's step reward, -inf where there is no candidate: lookahead's reward table, from the same launch
    that made the states."""
    rows = batch.n_envs if group is None else batch.group_bounds(group)[1] - batch.group_bounds(group)[0]
    k = max(int(batch.k_max), 1)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(batch.device)):
        values = torch.full((rows, k), float("-inf"), dtype=torch.float32, device=batch.device)
        rewards = torch.full((rows, k), float("-inf"), dtype=torch.float64, device=batch.device) if return_rewards else None
        for dims, sel, head, nlegal, region, reward, net in successor_states(batch, group, chunk, stream, groups):
            v = state_values(model, head, dims, ob_towers).reshape(int(sel.numel()), k)
            values.index_copy_(0, sel, _by_net(v, net, float("-inf")))
            if return_rewards:
                rewards.index_copy_(0, sel, _by_net(reward, net, float("-inf")))
    return (values, rewards) if return_rewards else values


def pick_best(scores: torch.Tensor) -> torch.Tensor:
    """int32 [rows]: the net (column + 1) of the highest score of every row, ties to the lowest net (the first maximum; argmax does
    not promise it); 0 where the row has no finite score (a done env)."""
    s = scores.to(torch.float64)
    s = torch.where(torch.isnan(s), torch.full_like(s, float("-inf")), s)
    best = s.max(dim=1, keepdim=True).values
    k = s.shape[1]
    idx = torch.arange(k, device=s.device).expand_as(s)
    first = torch.where((s == best) & (s > float("-inf")), idx, torch.full_like(idx, k)).min(dim=1).values
    return torch.where(first < k, first + 1, torch.zeros_like(first)).to(torch.int32)


@torch.no_grad()
def value_actions(model, batch, ob_towers=None, group: Optional[int] = None, chunk: int = DEFAULT_CHUNK, stream=None,
                  groups=None) -> torch.Tensor:
    """int32 actions [rows]: per env the net with the highest reward + value (the one-ply value-guided policy: the successor's step
    reward plus the critic's value of the successor state, added in float64), ties to the lowest net, 0 for a done env."""
    values, rewards = successor_values(model, batch, ob_towers, group, chunk, stream, return_rewards=True, groups=groups)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(batch.device)):
        return pick_best(rewards + values.to(torch.float64))


def value_prior(values: torch.Tensor, rewards: torch.Tensor, temperature: float = 1.0):
    """(prior fp32 [rows, k_max], sim_weights int32 [rows, k_max]) for tree_search(prior=..., sim_weights=...) from net-indexed values
    and rewards (successor_values(return_rewards=True), or lookahead's reward table).  The score of a candidate is reward + value in
    float64, divided by the spread of its row (max - min over the candidates, at least 1); the prior is the softmax of the scores at
    `temperature` over the row's candidates (0 for nets that are no candidates; a row without candidates is all 0), the weights are
    envs.weighted.weights_from_scores of the same scores at the same temperature."""
    t = float(temperature)
    if not (t > 0.0 and t < float("inf")):
        raise ValueError(f"temperature must be finite and > 0, got {temperature}")
    s = rewards.to(torch.float64) + values.to(torch.float64)
    ok = torch.isfinite(s)
    hi = torch.where(ok, s, torch.full_like(s, float("-inf"))).max(dim=1, keepdim=True).values
    lo = torch.where(ok, s, torch.full_like(s, float("inf"))).min(dim=1, keepdim=True).values
    spread = torch.where(torch.isfinite(hi - lo), hi - lo, torch.ones_like(hi)).clamp_min(1.0)
    top = torch.where(torch.isfinite(hi), hi, torch.zeros_like(hi))
    z = torch.where(ok, (s - top) / spread, torch.full_like(s, float("-inf")))          # (<= 0 for every candidate)
    e = torch.where(ok, torch.exp(z / t), torch.zeros_like(z))
    prior = (e / e.sum(dim=1, keepdim=True).clamp_min(1e-300)).to(torch.float32).contiguous()
    return prior, weights_from_scores(z, t).contiguous()
