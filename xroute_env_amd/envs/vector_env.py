"""Batched env: B regions stepped per call on one MI355X, results left on the device.

This is the data-parallel form of Game.step the north star asks for.  Nothing here synchronises with
the host: actions come in as a device tensor, observation / reward / done / legal masks stay device
tensors.  Envs that finished an episode are re-initialised by the next step (gym "next-step"
autoreset), with the reference's region rotation (examples/launch_training.py:28-54).

With `groups`, the slots are also split into env groups that step independently, each on a stream of its own
(`step_async` / `step_wait` / `poll` / `ready_groups`): the worker model of the reference's A3C / MCTS trainers, whose
workers never wait for each other.  An env's trajectory depends only on its own actions, so any interleaving of group
steps gives, env by env, exactly what the lock-step `step()` gives.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from ..batch import RegionBatch, partition_bounds
from ..dist import RECORD_BYTES, unpack_records


class XRouteVectorEnv:
    def __init__(self, regions: Sequence, n_envs: Optional[int] = None, device="cuda:0", with_observation: bool = True,
                 dict_observation: bool = False, groups=None, obs_dtype=torch.float32, **batch_kw):
        """dict_observation: reset() / step() return the observation as the advertised Dict space's member
        {"grid": [B, stride] fp32, "legal_mask": [B, Kmax] u8} instead of the bare grid tensor (the default: the hot loop's
        consumers — agents.dqn_actions / ppo_actions — take the grid buffer and the legal bitmasks of `info` as they are).
        groups: None (lock-step only, exactly as before), an int G (G near-equal env groups; at most 4 pay off where a process
        gets 4 hardware queues) or explicit bounds [0, ..., n_envs]: enables step_async / step_wait per group.
        obs_dtype: torch.float32 (default) or torch.uint8 — the same grid at one byte a value (a quarter of the bytes written per
        step and kept per transition; xr_batch_step_observe_u8), rows of obs_env_stride_u8 bytes."""
        if obs_dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"obs_dtype must be torch.float32 or torch.uint8, not {obs_dtype}")
        self.obs_dtype = obs_dtype
        self.batch = RegionBatch(regions, n_envs=n_envs, device=device, auto_reset=True, **batch_kw)
        self.n_envs = self.batch.n_envs
        self.device = self.batch.device
        self.with_observation = with_observation
        self.dict_observation = bool(dict_observation)
        # (zeros, not empty: a row beyond its env's (2+7K)*N floats then only ever holds zeros or stale 0/1 planes of earlier steps —
        #  inside the Box's bounds; consumers go by nlegal / legal_mask)
        self.obs = self.batch.alloc_observation(dtype=obs_dtype).zero_() if with_observation else None
        # the 48-byte xr_step_record of every env, written by the step / reset kernels themselves: ONE copy per step;
        # reward / done / delta / nlegal below are views into it
        self.record = torch.empty((self.n_envs, RECORD_BYTES), dtype=torch.uint8, device=self.device)
        rec = unpack_records(self.record)
        self.reward, self.delta, self.nlegal, self.cum = rec["reward"], rec["delta"], rec["nlegal"], rec["cum"]
        self.done = torch.empty(self.n_envs, dtype=torch.uint8, device=self.device)
        self.legal = torch.empty((self.n_envs, self.batch.legal_words), dtype=torch.int64, device=self.device)
        self.region = torch.empty(self.n_envs, dtype=torch.int32, device=self.device)
        # fixed-shape spaces (envs/spaces.py): grid rows are the device buffer's own flat rows [B, stride >= (2+7*Kmax)*N]
        from . import spaces as xr_spaces
        self.kmax = max(self.batch.k_max, 1)
        dims = set(tuple(int(v) for v in r.dims) for r in self.batch.regions)
        self.single_observation_space = self.single_action_space = self.observation_space = self.action_space = None
        if len(dims) == 1:
            d = dims.pop()
            u8 = obs_dtype == torch.uint8
            dt = np.uint8 if u8 else None
            self.single_observation_space, self.single_action_space = xr_spaces.fixed_spaces(d, self.kmax, dtype=dt)
            row = int(self.batch.obs_env_stride_u8 if u8 else self.batch.obs_env_stride)
            self.observation_space, _ = xr_spaces.fixed_spaces(d, self.kmax, batch=self.n_envs, row=row, dtype=dt)
            self.action_space = self.single_action_space
        # env groups: one stream and one completion event per group; group g's rows are views [lo:hi] of the buffers above
        self.group_streams, self.group_events = [], []
        self.n_groups = 0
        if groups is not None:
            self.batch.set_groups(partition_bounds(groups, self.n_envs))
            self.n_groups = self.batch.n_groups
            self.group_streams = [torch.cuda.Stream(device=self.device) for _ in range(self.n_groups)]
            self.group_events = [torch.cuda.Event() for _ in range(self.n_groups)]

    def observation_dict(self) -> dict:
        """The current observation as a member of `observation_space`: the grid buffer itself (no copy) + the legal mask."""
        return {"grid": self.obs, "legal_mask": self.legal_mask()}

    def legal_mask(self) -> torch.Tensor:
        """uint8 [B, Kmax] (the `legal_mask` of the Dict space): bit n-1 of an env's row <=> net n is in its netSet; a device op on
        the bitmasks of the last step / reset."""
        bits = torch.arange(64, device=self.device, dtype=torch.int64)
        m = ((self.legal.unsqueeze(-1) >> bits) & 1).reshape(self.n_envs, -1)
        return m[:, :self.kmax].to(torch.uint8)

    def _collect(self, observe: bool):
        b = self.batch
        if observe and self.with_observation:
            b.observation(self.obs)
        b.fetch("record", self.record)
        b.fetch("done", self.done)
        b.fetch("legal", self.legal)
        b.fetch("region", self.region)          # the region every slot is playing (key of agents.NetVectorCache)
        return (self.observation_dict() if self.dict_observation and self.with_observation else self.obs), self.reward, self.done, {"delta": self.delta, "nlegal": self.nlegal, "legal": self.legal,
                                                  "region": self.region, "record": self.record, "cum": self.cum}

    def _join_groups(self):
        """Order the current stream after every group's outstanding work (a whole-batch call follows all of it)."""
        cur = torch.cuda.current_stream(self.device)
        for ev in self.group_events:
            cur.wait_event(ev)

    def reset(self):
        self._join_groups()
        self.batch.reset(rotate=True)
        obs, _, _, info = self._collect(observe=True)
        return obs, info

    def step(self, actions: torch.Tensor):
        self._join_groups()
        if self.with_observation:
            # route + observation of every env; self.obs is this env's own persistent buffer, so the in-place form applies:
            # only the planes that change are written (byte-identical to a full write; do not write into `obs` yourself)
            self.batch.step(actions, self.obs, inplace=True)
            return self._collect(observe=False)
        self.batch.step(actions)
        return self._collect(observe=False)

    def random_actions(self, seed: int, out: Optional[torch.Tensor] = None):
        return self.batch.random_actions(seed, out)

    def weighted_actions(self, weights: torch.Tensor, seed: int, out: Optional[torch.Tensor] = None, group: Optional[int] = None):
        """RegionBatch.weighted_actions: a legal net per env drawn in proportion to weights (int32 [rows, k_max]); unit weights are
        random_actions(seed).  group None: the whole batch, after every group's outstanding work.  A group: on that group's stream,
        ordered like lookahead(group); the group's event then covers it."""
        if group is None:
            self._join_groups()
            return self.batch.weighted_actions(weights, seed, out)
        (g,) = self._groups_of(group)
        s = self.group_streams[g]
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            res = self.batch.weighted_actions(weights, seed, out, group=g, stream=s)
            self.group_events[g].record(s)
        return res

    # ---- lookahead: every candidate net priced from the current state, the env untouched ------------------------------------------
    def lookahead(self, group: Optional[int] = None):
        """(delta_status int32 [rows, k_max, 4], reward float64 [rows, k_max]) of RegionBatch.lookahead: what step() would publish for
        every net an env may pick now (-1 status / -inf reward where a net is no candidate).  group None: the whole batch, after every
        group's outstanding work.  A group: on that group's stream, after the current stream and the group's last step; the group's
        event then covers it, so step_wait(group) / poll(group) order a consumer after the result."""
        if group is None:
            self._join_groups()
            return self.batch.lookahead()
        (g,) = self._groups_of(group)
        s = self.group_streams[g]
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            res = self.batch.lookahead(group=g, stream=s)
            self.group_events[g].record(s)
        return res

    def greedy_actions(self, group: Optional[int] = None) -> torch.Tensor:
        """int32 actions [rows]: per env the net with the highest lookahead reward (the cheapest next route), the first maximum in
        ascending net id; 0 for a done env, like random_actions."""
        if group is None:
            _, reward = self.lookahead()
            return self._argmax_first(reward)
        (g,) = self._groups_of(group)
        _, reward = self.lookahead(g)
        s = self.group_streams[g]
        with torch.cuda.stream(s):
            act = self._argmax_first(reward)
            self.group_events[g].record(s)
        return act

    @staticmethod
    def _argmax_first(reward: torch.Tensor) -> torch.Tensor:
        best = reward.max(dim=1, keepdim=True).values
        k = reward.shape[1]
        idx = torch.arange(k, device=reward.device).expand_as(reward)
        first = torch.where(reward == best, idx, torch.full_like(idx, k)).min(dim=1).values      # (argmax does not promise the first maximum)
        return torch.where(best.squeeze(1) == float("-inf"), torch.zeros_like(first), first + 1).to(torch.int32)

    # ---- rollouts: every env's episode played to its end from the current state, the env untouched ---------------------------------
    def rollout(self, n_rollouts: int, seed: int = 0, policy="random", prefix: Optional[torch.Tensor] = None, max_plies: int = 0,
                group: Optional[int] = None, weights: Optional[torch.Tensor] = None):
        """RegionBatch.rollout's dict {out, ret, hash, order}.  group None: the whole batch, after every group's outstanding work.  A
        group: on that group's stream, ordered like lookahead(group); the group's event then covers it.  weights: with
        policy="weighted", int32 [rows, k_max]."""
        if group is None:
            self._join_groups()
            return self.batch.rollout(n_rollouts, seed, policy, prefix, max_plies, weights=weights)
        (g,) = self._groups_of(group)
        s = self.group_streams[g]
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            res = self.batch.rollout(n_rollouts, seed, policy, prefix, max_plies, group=g, stream=s, weights=weights)
            self.group_events[g].record(s)
        return res

    def peek(self, prefix: Optional[torch.Tensor], n_lines: Optional[int] = None, max_plies: int = 0, region_base: int = 0,
             row_bytes: Optional[int] = None, group: Optional[int] = None):
        """RegionBatch.peek's dict {rows, out, ret, hash, order}: the packed state after each line of play, without stepping.  group
        None: the whole batch, after every group's outstanding work.  A group: on that group's stream, ordered like rollout(group); the
        group's event then covers it."""
        if group is None:
            self._join_groups()
            return self.batch.peek(prefix, n_lines, max_plies, region_base, row_bytes)
        (g,) = self._groups_of(group)
        s = self.group_streams[g]
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            res = self.batch.peek(prefix, n_lines, max_plies, region_base, row_bytes, group=g, stream=s)
            self.group_events[g].record(s)
        return res

    def rollout_actions(self, n_rollouts: int, seed: int, group: Optional[int] = None) -> torch.Tensor:
        """int32 actions [rows]: per env the first net of its best random rollout (the highest return of n_rollouts; the first maximum
        on a tie); 0 for a done env, like random_actions."""
        if group is None:
            return self._first_of_best(self.rollout(n_rollouts, seed))
        (g,) = self._groups_of(group)
        res = self.rollout(n_rollouts, seed, group=g)
        s = self.group_streams[g]
        with torch.cuda.stream(s):
            act = self._first_of_best(res)
            self.group_events[g].record(s)
        return act

    @staticmethod
    def _first_of_best(res) -> torch.Tensor:
        ret, first = res["ret"], res["order"][:, :, 0]
        best = ret.max(dim=1, keepdim=True).values
        R = ret.shape[1]
        idx = torch.arange(R, device=ret.device).expand_as(ret)
        r = torch.where(ret == best, idx, torch.full_like(idx, R)).min(dim=1, keepdim=True).values      # (the first maximum)
        return first.gather(1, r).squeeze(1).to(torch.int32)          # (a done env's orders are all 0)

    # ---- branch: slots take other slots' state on the device -------------------------------------------------------------------------
    def branch(self, parent: torch.Tensor, group: Optional[int] = None) -> None:
        """RegionBatch.branch: row i continues from the state of row parent[i] (int32 [rows] on the device, relative to the group's first
        slot when `group` is given).  group None: the whole batch, after every group's outstanding work, as step().  A group: on that
        group's stream, after the current stream and the group's last work; the group's event then covers it.  The env's record / done /
        legal / region tensors are fetched again (the slots' rows moved); the observation buffer is not — the next step rewrites it in full,
        because a branch drops the in-place validity."""
        b = self.batch
        if group is None:
            self._join_groups()
            b.branch(parent)
            b.fetch("record", self.record)
            b.fetch("done", self.done)
            b.fetch("legal", self.legal)
            b.fetch("region", self.region)
            return
        (g,) = self._groups_of(group)
        lo, hi = b.group_bounds(g)
        s = self.group_streams[g]
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            b.branch(parent, group=g, stream=s)
            b.fetch_group("record", g, self.record[lo:hi], stream=s)
            b.fetch_group("done", g, self.done[lo:hi], stream=s)
            b.fetch_group("legal", g, self.legal[lo:hi], stream=s)
            b.fetch_group("region", g, self.region[lo:hi], stream=s)
            self.group_events[g].record(s)
        if isinstance(parent, torch.Tensor):
            parent.record_stream(s)

    # ---- tree search: MCTS over net orderings from the current state, the env untouched ------------------------------------------
    def tree_search(self, n_waves: int, n_par: int, seed: int = 0, prior: Optional[torch.Tensor] = None, node_cap: Optional[int] = None,
                    c_init: float = 1.25, c_base: float = 19652.0, group: Optional[int] = None, trace: bool = False,
                    sim_weights: Optional[torch.Tensor] = None, keep: bool = False, played: Optional[torch.Tensor] = None):
        """RegionBatch.tree_search's dict {visits, value, info, best_order, best_return[, paths, returns][, kept]}.  group None: the whole batch,
        after every group's outstanding work.  A group: on that group's stream, ordered like rollout(group); the group's event then
        covers it.  sim_weights: None, or int32 [rows, k_max]: the simulations follow the weighted policy.  keep, played: the kept search
        (RegionBatch.tree_search): the caller's tree stays, and continues where `played` says how its envs have moved."""
        if group is None:
            self._join_groups()
            return self.batch.tree_search(n_waves, n_par, seed, prior, node_cap, c_init, c_base, trace=trace, sim_weights=sim_weights, keep=keep,
                                          played=played)
        (g,) = self._groups_of(group)
        s = self.group_streams[g]
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            res = self.batch.tree_search(n_waves, n_par, seed, prior, node_cap, c_init, c_base, group=g, stream=s, trace=trace,
                                         sim_weights=sim_weights, keep=keep, played=played)
            self.group_events[g].record(s)
        if isinstance(played, torch.Tensor):
            played.record_stream(s)
        return res

    def tree_actions(self, n_waves: int, n_par: int, seed: int = 0, prior: Optional[torch.Tensor] = None, node_cap: Optional[int] = None,
                     c_init: float = 1.25, c_base: float = 19652.0, group: Optional[int] = None, keep: bool = False,
                     played: Optional[torch.Tensor] = None) -> torch.Tensor:
        """int32 actions [rows]: per env the most visited child of its search's root; ties go to the higher value, then to the lower
        net; 0 for a done env, like random_actions.  (A root that did not fit node_cap has no child: the first net of the best line.)
        keep, played: the kept search; the actions returned, once stepped, are the next call's `played`."""
        if group is None:
            return self._most_visited(self.tree_search(n_waves, n_par, seed, prior, node_cap, c_init, c_base, keep=keep, played=played))
        (g,) = self._groups_of(group)
        res = self.tree_search(n_waves, n_par, seed, prior, node_cap, c_init, c_base, group=g, keep=keep, played=played)
        s = self.group_streams[g]
        with torch.cuda.stream(s):
            act = self._most_visited(res)
            self.group_events[g].record(s)
        return act

    # ---- evaluated tree search (RegionBatch.tree_open / tree_leaves / tree_backup) --------------------------------------------------
    def _tree_eval_call(self, name: str, group, *args, **kw):
        """group None: the whole batch, after every group's outstanding work.  A group: on that group's stream, ordered like
        rollout(group); the group's event then covers it."""
        if group is None:
            self._join_groups()
            return getattr(self.batch, name)(*args, **kw)
        (g,) = self._groups_of(group)
        s = self.group_streams[g]
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            res = getattr(self.batch, name)(*args, group=g, stream=s, **kw)
            self.group_events[g].record(s)
        for t in list(args) + list(kw.values()):
            if isinstance(t, torch.Tensor):
                t.record_stream(s)
        return res

    def tree_open(self, n_par: int, max_sims: int, root_prior: Optional[torch.Tensor] = None, node_cap: Optional[int] = None,
                  c_init: float = 1.25, c_base: float = 19652.0, group: Optional[int] = None, keep: bool = False,
                  played: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """RegionBatch.tree_open: start an evaluated-tree session from the state the envs (of the group) are in now.  keep, played: the
        kept session (xr_batch_tree_reopen): it continues where `played` says how its envs have moved, and returns `kept`."""
        return self._tree_eval_call("tree_open", group, n_par, max_sims, root_prior, node_cap, c_init, c_base, keep=keep, played=played)

    def tree_leaves(self, region_base: int = 0, row_bytes: Optional[int] = None, group: Optional[int] = None):
        """RegionBatch.tree_leaves's dict {rows, out, ret, paths, leaf}: one wave's leaves as packed state rows."""
        return self._tree_eval_call("tree_leaves", group, region_base, row_bytes)

    def tree_backup(self, value: torch.Tensor, leaf_prior: Optional[torch.Tensor] = None, group: Optional[int] = None):
        """RegionBatch.tree_backup's dict {visits, value, info, best_order, best_return, returns}: the evaluator's values go into the tree."""
        return self._tree_eval_call("tree_backup", group, value, leaf_prior)

    @staticmethod
    def _most_visited(res) -> torch.Tensor:
        visits, value = res["visits"], res["value"]
        k = visits.shape[1]
        top = visits.max(dim=1, keepdim=True).values
        cand = (visits == top) & (visits > 0)
        val = torch.where(cand, value, torch.full_like(value, float("-inf")))
        best = val.max(dim=1, keepdim=True).values
        idx = torch.arange(k, device=visits.device).expand_as(visits)
        first = torch.where(cand & (val == best), idx, torch.full_like(idx, k)).min(dim=1).values          # (the lowest net of the tie)
        # no visited child: a done env (its best order is all 0), or a pool too small for the root (the first net of the best line seen)
        return torch.where(first == k, res["best_order"][:, 0].to(first.dtype), first + 1).to(torch.int32)

    # ---- independent stepping of env groups -----------------------------------------------------------------------------
    def _groups_of(self, group):
        if not self.n_groups:
            raise RuntimeError("step_async / step_wait / poll need XRouteVectorEnv(..., groups=...)")
        if group is None:
            return range(self.n_groups)
        g = int(group)
        if not 0 <= g < self.n_groups:
            raise ValueError(f"group {group} outside 0..{self.n_groups - 1}")
        return (g,)

    def step_async(self, actions: torch.Tensor, group: Optional[int] = None):
        """Enqueue the step of `group` (None: every group, each on its own stream) and return at once.  actions: int32 on the device,
        the group's own [hi - lo] entries or all n_envs (the group's rows are taken).  The group's stream first waits for the current
        stream (where the actions were made); collect the result with step_wait(group)."""
        if actions.device != self.device or actions.dtype != torch.int32 or not actions.is_contiguous():
            raise ValueError("actions must be a contiguous int32 tensor on the env's device")
        groups = self._groups_of(group)
        cur = torch.cuda.current_stream(self.device)
        b = self.batch
        for g in groups:
            lo, hi = b.group_bounds(g)
            if actions.numel() == self.n_envs:
                act = actions[lo:hi]
            elif group is not None and actions.numel() == hi - lo:
                act = actions
            else:
                raise ValueError(f"actions must have n_envs = {self.n_envs} entries" + ("" if group is None else f" or the group's {hi - lo}"))
            s = self.group_streams[g]
            s.wait_stream(cur)
            with torch.cuda.stream(s):
                if self.with_observation:
                    b.step_group(g, act, self.obs[lo:hi], inplace=True, stream=s)
                else:
                    b.step_group(g, act, stream=s)
                b.fetch_group("record", g, self.record[lo:hi], stream=s)
                b.fetch_group("done", g, self.done[lo:hi], stream=s)
                b.fetch_group("legal", g, self.legal[lo:hi], stream=s)
                b.fetch_group("region", g, self.region[lo:hi], stream=s)
                self.group_events[g].record(s)
            act.record_stream(s)                   # (the caching allocator must not hand the actions' memory out before s has read them)

    def step_wait(self, group: Optional[int] = None):
        """Make the current stream wait for the last step_async of `group` (None: every group) and return its
        (obs, reward, done, info): views of rows [lo:hi] of the env's buffers — for group None exactly what step() returns."""
        groups = self._groups_of(group)
        cur = torch.cuda.current_stream(self.device)
        for g in groups:
            cur.wait_event(self.group_events[g])
        if group is None:
            return self._result(slice(0, self.n_envs))
        lo, hi = self.batch.group_bounds(groups[0])
        return self._result(slice(lo, hi))

    def _result(self, sl: slice):
        """(obs, reward, done, info) of rows `sl`: step()'s own tensors for the whole batch, views of them for a group."""
        v = (lambda t: t) if (sl.start == 0 and sl.stop == self.n_envs) else (lambda t: t[sl])
        obs = self.obs if self.obs is None else v(self.obs)
        if self.dict_observation and self.with_observation:
            obs = {"grid": obs, "legal_mask": v(self.legal_mask())}
        info = {"delta": v(self.delta), "nlegal": v(self.nlegal), "legal": v(self.legal), "region": v(self.region),
                "record": v(self.record), "cum": v(self.cum)}
        return obs, v(self.reward), v(self.done), info

    def poll(self, group: int) -> bool:
        """True when the last step_async of `group` has finished on the device (non-blocking)."""
        (g,) = self._groups_of(group)
        return bool(self.group_events[g].query())

    def ready_groups(self):
        """The groups whose last step has finished (non-blocking)."""
        return [g for g in range(self.n_groups) if self.group_events[g].query()]
