"""RegionBatch — Python host layer over the `xr_batch_*` C ABI (include/xroute_hip.h).

A batch holds B env slots on one MI355X.  torch is plumbing only: it allocates the caller-side
device buffers (actions, observation, fetched results) and supplies the HIP stream; all compute is in
libxroute_hip.so.  One process per GPU; see xroute_env_amd/dist.py for the sharded launcher.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .regions import Region


RECORD_DTYPE = np.dtype([("reward", "<f8"), ("delta", "<i4", (3,)), ("cum", "<i4", (3,)), ("nlegal", "<i4"),
                         ("env_steps", "<i4"), ("path_len", "<i4"), ("done", "u1"), ("pad", "u1"), ("status", "<u2")])
assert RECORD_DTYPE.itemsize == _lib.RECORD_BYTES


def _require_gpu(device) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("xroute_env_amd needs a HIP device (MI355X): torch.cuda.is_available() is False "
                           "and there is no CPU fallback")
    return dev


def _stream_ptr(dev) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def partition_bounds(groups, n_envs: int) -> List[int]:
    """Env-group bounds [0, b1, ..., n_envs] of `groups`: an int G (G near-equal contiguous groups) or explicit ascending bounds.
    Raises ValueError for what xr_batch_set_groups would refuse: empty groups, bounds not from 0 to n_envs, more than XR_MAX_GROUPS."""
    n_envs = int(n_envs)
    if isinstance(groups, bool):
        raise ValueError("groups must be an int or a sequence of bounds, not a bool")
    if isinstance(groups, (int, np.integer)):
        g = int(groups)
        if g < 1 or g > min(n_envs, _lib.XR_MAX_GROUPS):
            raise ValueError(f"groups must be in 1..min(n_envs = {n_envs}, {_lib.XR_MAX_GROUPS}), got {g}")
        return [(i * n_envs) // g for i in range(g + 1)]
    b = [int(v) for v in groups]
    if len(b) < 2 or len(b) - 1 > _lib.XR_MAX_GROUPS:
        raise ValueError(f"bounds must hold 2..{_lib.XR_MAX_GROUPS + 1} values (n_groups + 1), got {len(b)}")
    if b[0] != 0 or b[-1] != n_envs:
        raise ValueError(f"bounds must run from 0 to n_envs = {n_envs}, got {b[0]} .. {b[-1]}")
    if any(hi <= lo for lo, hi in zip(b, b[1:])):
        raise ValueError("bounds must be strictly ascending: no group may be empty")
    return b


class RegionBatch:
    """B env slots playing a set of regions.  Mirrors, per env, the reference's Game
    (baseline/baseline_utils.py:383-481): reset() / step(actions) / observation()."""

    def __init__(self, regions: Sequence[Region], n_envs: Optional[int] = None, device="cuda:0",
                 auto_reset: bool = False, via_cost: int = 800, drc_cost: int = 8, drc_unit: int = 400,
                 max_route_count: int = 10, path_cap: int = 0, block_threads: int = 0,
                 force_scratch_field: bool = False, obs_mode: int = 0, obs_writer_blocks: int = 0,
                 obs_split_permille: int = 0, router: int = 0, dial_mult: int = 0,
                 stream_per_region: bool = False, obs_helper_blocks: int = 0, launch_order: int = 0,
                 guide_cost: int = 0, guide_margin: int = 0, maze_end_iter: int = 1, debug_round_cap: int = 0,
                 window: int = 0):
        self.device = _require_gpu(device)
        self.L = _lib.lib()
        self.regions = list(regions)
        self.n_envs = int(n_envs if n_envs is not None else len(self.regions))
        cfg = _lib.default_config()
        cfg.device = self.device.index if self.device.index is not None else torch.cuda.current_device()
        cfg.n_envs = self.n_envs
        cfg.via_cost, cfg.drc_cost, cfg.drc_unit = via_cost, drc_cost, drc_unit
        cfg.max_route_count = max_route_count
        cfg.auto_reset = int(auto_reset)
        cfg.path_cap = path_cap
        cfg.block_threads = block_threads
        cfg.force_scratch_field = int(force_scratch_field)
        cfg.obs_mode = int(obs_mode)                    # 0 default, 1 fused single launch, 2 split (route || net-plane writer)
        cfg.obs_writer_blocks = int(obs_writer_blocks)
        cfg.obs_split_permille = int(obs_split_permille)   # split form: share of the net planes the writer kernel takes
        cfg.router = int(router)                        # 0 auto (frontier router; the full-rewrite queue launch of >= 4096 slots takes the sweeps), 1 line-segment sweeps, 2 frontier (required)
        cfg.dial_mult = int(dial_mult)
        cfg.launch_order = int(launch_order)             # route-only launches: 0 auto, 1 slot order, 2 longest predicted route first
        cfg.obs_helper_blocks = int(obs_helper_blocks)   # queue form: LDS-free helper writers beside the step kernel (0 = none = the default; < 0 is rejected)
        cfg.debug_round_cap = int(debug_round_cap)       # 0 default (1024 + N rounds per search); tests force XR_ENV_ROUTER_ABORT with 1
        cfg.guide_cost, cfg.guide_margin, cfg.maze_end_iter = int(guide_cost), int(guide_margin), int(maze_end_iter)   # XR-Maze v2
        cfg.window = int(window)                         # regions too large for LDS: > 0 = LDS-window router first (at most that many tracks); 0 = off (measured no faster)
        cfg.stream_per_region = int(stream_per_region)   # one single-workgroup launch per env slot on a pool of streams (<= 64 slots)
        self.cfg = cfg
        self.region_epoch = 0      # bumped whenever the HOST changes which region a slot plays (assign, reset(rotate), load_state_dict)
        self._h = C.c_void_p()
        _lib.check(self.L.xr_batch_create(C.byref(cfg), C.byref(self._h)))
        with torch.cuda.device(self.device):
            self._load()

    # ------------------------------------------------------------------------------------------
    def _load(self):
        descs = (_lib.XrRegionDesc * len(self.regions))()
        keep = []
        for i, r in enumerate(self.regions):
            xs = np.ascontiguousarray(r.xs, np.int32)
            ys = np.ascontiguousarray(r.ys, np.int32)
            ld = np.ascontiguousarray(r.layer_dir, np.uint8)
            nd = np.ascontiguousarray(r.nodes, np.uint32)
            if nd.size != r.n_nodes:
                raise ValueError(f"region {i}: {nd.size} node records for dims {r.dims}")
            keep += [xs, ys, ld, nd]
            d = descs[i]
            d.dim_x, d.dim_y, d.dim_z = (int(v) for v in r.dims)
            d.xs_host, d.ys_host = xs.ctypes.data, ys.ctypes.data
            d.layer_dir_host, d.nodes_host = ld.ctypes.data, nd.ctypes.data
            d.n_nets = int(r.n_nets)
            for j in range(3):
                d.metrics0[j] = int(r.metrics0[j])
        _lib.check(self.L.xr_batch_load_regions(self._h, descs, len(self.regions), _stream_ptr(self.device)))
        self._load_guides()
        sz = [C.c_int32() for _ in range(6)]
        stride = C.c_int64()
        _lib.check(self.L.xr_batch_sizes(self._h, *[C.byref(s) for s in sz], C.byref(stride)))
        (_, self.n_regions, self.n_max, self.k_max, self.legal_words, self.path_cap) = (s.value for s in sz)
        self.obs_env_stride = stride.value

    def _load_guides(self):
        """XR-Maze v2: regions that carry global-route guide boxes (`Region.guide_off / guide_box`, lefdef.RegionExtractor) hand
        them to the device (xr_batch_load_guides); the others keep the default guide (bounding box of the net's access points)."""
        if not any(getattr(r, "guide_off", None) is not None for r in self.regions):
            return
        n = len(self.regions)
        offs, boxes, keep = (C.c_void_p * n)(), (C.c_void_p * n)(), []
        for i, r in enumerate(self.regions):
            if getattr(r, "guide_off", None) is None:
                continue
            off = np.ascontiguousarray(r.guide_off, np.int32)
            box = np.ascontiguousarray(r.guide_box, np.int16).reshape(-1, 6)
            if off.size != r.n_nets + 1 or int(off[-1]) != box.shape[0]:
                raise ValueError(f"region {i}: guide_off must have n_nets + 1 entries and end at the number of boxes")
            if box.shape[0] == 0:
                box = np.zeros((1, 6), np.int16)
            keep += [off, box]
            offs[i], boxes[i] = off.ctypes.data, box.ctypes.data
        _lib.check(self.L.xr_batch_load_guides(self._h, offs, boxes, _stream_ptr(self.device)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self.L.xr_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------
    def assign(self, env_region: Sequence[int]):
        a = np.ascontiguousarray(env_region, np.int32)
        if a.size != self.n_envs:
            raise ValueError("env_region must have n_envs entries")
        _lib.check(self.L.xr_batch_assign(self._h, a.ctypes.data))
        self.region_epoch += 1

    def reset(self, mask: Optional[torch.Tensor] = None, rotate: bool = False):
        """Game.reset for the masked envs (all when mask is None)."""
        ptr = None
        if mask is not None:
            mask = mask.to(device=self.device, dtype=torch.uint8).contiguous()
            if mask.numel() != self.n_envs:
                raise ValueError("mask must have n_envs entries")
            ptr = C.c_void_p(mask.data_ptr())
        with torch.cuda.device(self.device):
            _lib.check(self.L.xr_batch_reset(self._h, ptr, int(rotate), _stream_ptr(self.device)))
        self.region_epoch += int(bool(rotate))

    def step(self, actions: torch.Tensor, obs_out: Optional[torch.Tensor] = None, inplace: bool = False):
        """Game.step for every env: actions int32[B] on the device, 1-based net ids.  With `obs_out`
        ([n_envs, stride] fp32) the same launch also writes every env's observation of the new state
        (xr_batch_step_observe).  `inplace=True` (xr_batch_step_observe_inplace): `obs_out` is the buffer that received this
        batch's previous observation and has not been written to since — only the planes that change are written."""
        if actions.device != self.device or actions.dtype != torch.int32 or not actions.is_contiguous() \
                or actions.numel() != self.n_envs:
            raise ValueError("actions must be a contiguous int32 tensor of n_envs entries on the batch device")
        with torch.cuda.device(self.device):
            if obs_out is None:
                _lib.check(self.L.xr_batch_step(self._h, C.c_void_p(actions.data_ptr()), _stream_ptr(self.device)))
            else:
                self._check_obs(obs_out, self.n_envs, "obs_out")
                if obs_out.dtype == torch.uint8:           # the same step, the observation as bytes (xr_batch_step_observe_u8)
                    _lib.check(self.L.xr_batch_step_observe_u8(self._h, -1, C.c_void_p(actions.data_ptr()), C.c_void_p(obs_out.data_ptr()),
                                                               obs_out.shape[1], _lib.XR_OBS_U8_INPLACE if inplace else 0,
                                                               _stream_ptr(self.device)))
                    return obs_out
                fn = self.L.xr_batch_step_observe_inplace if inplace else self.L.xr_batch_step_observe
                _lib.check(fn(self._h, C.c_void_p(actions.data_ptr()), C.c_void_p(obs_out.data_ptr()), obs_out.shape[1],
                              _stream_ptr(self.device)))
        return obs_out

    # ---- env groups: subsets of the slots stepped independently, each on its own stream (include/xroute_hip.h) ------------------
    def set_groups(self, bounds):
        """Partition the slots into env groups: `bounds` = [0, b1, ..., n_envs] strictly ascending, or an int G (near-equal groups).
        No work of the batch may be in flight (xr_batch_set_groups may synchronise)."""
        b = np.ascontiguousarray(partition_bounds(bounds, self.n_envs), np.int32)
        with torch.cuda.device(self.device):
            _lib.check(self.L.xr_batch_set_groups(self._h, b.ctypes.data, b.size - 1))
        self._group_bounds = [int(v) for v in b]
        self._tree_sessions = {}          # (an evaluated-tree session belongs to the rows it was opened for)

    @property
    def n_groups(self) -> int:
        return len(self._bounds()) - 1

    def _bounds(self) -> List[int]:
        return getattr(self, "_group_bounds", None) or [0, self.n_envs]

    def group_bounds(self, g: int):
        """(lo, hi): group g is slots [lo, hi)."""
        b = self._bounds()
        if not 0 <= int(g) < len(b) - 1:
            raise ValueError(f"group {g} outside 0..{len(b) - 2}")
        return b[int(g)], b[int(g) + 1]

    def _stream_arg(self, stream) -> C.c_void_p:
        return C.c_void_p((stream if stream is not None else torch.cuda.current_stream(self.device)).cuda_stream)

    def step_group(self, g: int, actions: torch.Tensor, obs_out: Optional[torch.Tensor] = None, inplace: bool = False, stream=None):
        """step() for the envs of group g only (xr_batch_step_group), enqueued on `stream` (default: the current stream): actions int32
        [hi - lo] (entry i = env lo + i); obs_out ([hi - lo, stride] fp32, e.g. rows lo:hi of the batch's buffer) receives env lo + i's
        observation in row i.  `inplace`: obs_out holds the group's previous observation (the in-place form, validity tracked per group)."""
        lo, hi = self.group_bounds(g)
        if actions.device != self.device or actions.dtype != torch.int32 or not actions.is_contiguous() or actions.numel() != hi - lo:
            raise ValueError("actions must be a contiguous int32 tensor of the group's size on the batch device")
        out_ptr, stride = None, 0
        if obs_out is not None:
            if obs_out.device != self.device or obs_out.dtype not in (torch.float32, torch.uint8) or not obs_out.is_contiguous() \
                    or obs_out.dim() != 2 or obs_out.shape[0] < hi - lo:
                raise ValueError("obs_out must be a contiguous fp32 or uint8 [group size, stride] tensor on the batch device")
            out_ptr, stride = C.c_void_p(obs_out.data_ptr()), int(obs_out.shape[1])
            if obs_out.dtype == torch.uint8:
                with torch.cuda.device(self.device):
                    _lib.check(self.L.xr_batch_step_observe_u8(self._h, int(g), C.c_void_p(actions.data_ptr()), out_ptr, stride,
                                                               _lib.XR_OBS_U8_INPLACE if inplace else 0, self._stream_arg(stream)))
                return obs_out
        flags = _lib.XR_GROUP_INPLACE if (inplace and obs_out is not None) else 0
        with torch.cuda.device(self.device):
            _lib.check(self.L.xr_batch_step_group(self._h, int(g), C.c_void_p(actions.data_ptr()), out_ptr, stride, flags,
                                                  self._stream_arg(stream)))
        return obs_out

    def random_actions_group(self, g: int, seed: int, out: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
        """random_actions() for the envs of group g: out int32 [hi - lo], entry i = env lo + i."""
        lo, hi = self.group_bounds(g)
        if out is None:
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
                out = torch.empty(hi - lo, dtype=torch.int32, device=self.device)
        if out.device != self.device or out.dtype != torch.int32 or not out.is_contiguous() or out.numel() != hi - lo:
            raise ValueError("out must be a contiguous int32 tensor of the group's size on the batch device")
        with torch.cuda.device(self.device):
            _lib.check(self.L.xr_batch_random_actions_group(self._h, int(g), C.c_void_p(out.data_ptr()), C.c_uint64(seed & (2 ** 64 - 1)),
                                                            self._stream_arg(stream)))
        return out

    # the per-env arrays xr_batch_fetch_group copies
    _GROUP_FETCH = ("record", "reward", "done", "nlegal", "status", "legal", "delta", "cum", "path_len", "path", "owner", "hash", "region",
                    "sweeps", "replay", "env_steps")

    def fetch_group(self, what: str, g: int, out: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
        """fetch() of group g's rows of a per-env array (async on `stream`, default the current stream)."""
        if what not in self._GROUP_FETCH:
            raise ValueError(f"fetch_group: {what!r} is not a per-env array ({', '.join(self._GROUP_FETCH)})")
        sel, dtype, shape = self._FETCH[what]
        lo, hi = self.group_bounds(g)
        shp = (hi - lo,) + tuple(shape(self))[1:]
        if out is None:
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
                out = torch.empty(shp, dtype=dtype, device=self.device)
        if out.dtype != dtype or not out.is_contiguous() or tuple(out.shape) != shp:
            raise ValueError(f"out must be a contiguous {dtype} tensor of shape {shp}")
        with torch.cuda.device(self.device):
            _lib.check(self.L.xr_batch_fetch_group(self._h, int(g), sel, C.c_void_p(out.data_ptr()), out.numel() * out.element_size(),
                                                   self._stream_arg(stream)))
        return out

    # ---- lookahead: what every candidate net would cost, without stepping (xr_batch_lookahead) ---------------------------------
    def lookahead(self, mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, reward_out: Optional[torch.Tensor] = None,
                  group: Optional[int] = None, stream=None):
        """From the state every env is in now, price every net it may still pick; the batch is left exactly as it was.  Returns
        (delta_status int32 [rows, k_max, 4], reward float64 [rows, k_max]) as device tensors: entry n - 1 of an env's row holds
        {d_violation, d_wirelength, d_via, status} and the reward step() would publish if net n were its action now; nets that are not
        candidates hold {0, 0, 0, -1} and -inf (an arg-max over a reward row is the greedy action; a done env has no candidate).
        mask: optional int64 / uint64 [rows, legal_words] bitmasks, the candidates are legal & mask.  group: an env group (rows = its
        slots, enqueued on `stream`, default the current stream); None: the whole batch."""
        if group is None:
            g, rows = -1, self.n_envs
        else:
            lo, hi = self.group_bounds(group)
            g, rows = int(group), hi - lo
        k = max(int(self.k_max), 1)
        if out is None or reward_out is None:
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
                out = torch.empty((rows, k, 4), dtype=torch.int32, device=self.device) if out is None else out
                reward_out = torch.empty((rows, k), dtype=torch.float64, device=self.device) if reward_out is None else reward_out
        if out.device != self.device or out.dtype != torch.int32 or not out.is_contiguous() or tuple(out.shape) != (rows, k, 4):
            raise ValueError(f"out must be a contiguous int32 [{rows}, {k}, 4] tensor on the batch device")
        if reward_out.device != self.device or reward_out.dtype != torch.float64 or not reward_out.is_contiguous() \
                or tuple(reward_out.shape) != (rows, k):
            raise ValueError(f"reward_out must be a contiguous float64 [{rows}, {k}] tensor on the batch device")
        mp = None
        if mask is not None:
            if mask.device != self.device or mask.dtype not in (torch.int64, torch.uint64) or not mask.is_contiguous() \
                    or tuple(mask.shape) != (rows, self.legal_words):
                raise ValueError(f"mask must be a contiguous 64-bit [{rows}, {self.legal_words}] tensor on the batch device")
            mp = C.c_void_p(mask.data_ptr())
        with torch.cuda.device(self.device):
            _lib.check(self.L.xr_batch_lookahead(self._h, g, mp, C.c_void_p(out.data_ptr()), k, C.c_void_p(reward_out.data_ptr()),
                                                 self._stream_arg(stream)))
        return out, reward_out

    # ---- weighted net sampling: a legal net in proportion to per-net integer weights (xr_batch_weighted_actions, XR-Pick v1) ----
    def weighted_actions(self, weights: torch.Tensor, seed: int, out: Optional[torch.Tensor] = None, group: Optional[int] = None,
                         stream=None) -> torch.Tensor:
        """random_actions() under per-net weights: action i is drawn from the legal nets of row i with probability proportional to
        weights[i, net - 1] (int32 [rows, k_max]; <= 0 counts as 0, values are clamped to XR_WEIGHT_MAX = 2^24; when every legal net
        counts 0 the pick is the uniform one).  Exact in integers and keyed by (seed, global env index, env_steps) like random_actions:
        unit weights give random_actions(seed) bit for bit.  0 for a done env.  group: an env group (rows = its slots, enqueued on
        `stream`, default the current stream); None: the whole batch."""
        if group is None:
            g, rows = -1, self.n_envs
        else:
            lo, hi = self.group_bounds(group)
            g, rows = int(group), hi - lo
        wp = self._check_weights(weights, rows)
        if out is None:
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
                out = torch.empty(rows, dtype=torch.int32, device=self.device)
        if not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype != torch.int32 or not out.is_contiguous() \
                or tuple(out.shape) != (rows,):
            raise ValueError(f"out must be a contiguous int32 [{rows}] tensor on the batch device")
        with torch.cuda.device(self.device):
            _lib.check(self.L.xr_batch_weighted_actions(self._h, g, wp, max(int(self.k_max), 1), C.c_void_p(out.data_ptr()),
                                                        C.c_uint64(int(seed) & (2 ** 64 - 1)), self._stream_arg(stream)))
        return out

    # ---- rollouts: every env's episode played to its end, without stepping (xr_batch_rollout) -----------------------------------
    _ROLLOUT_POLICY = {"stop": _lib.XR_ROLLOUT_STOP, "random": _lib.XR_ROLLOUT_RANDOM, "weighted": _lib.XR_ROLLOUT_WEIGHTED}

    def _check_weights(self, weights, rows: int, name: str = "weights") -> C.c_void_p:
        """A weight table of XR-Pick v1: contiguous int32 [rows, k_max] on the batch device (net n at column n - 1)."""
        k = max(int(self.k_max), 1)
        if not isinstance(weights, torch.Tensor) or weights.device != self.device or weights.dtype != torch.int32 or not weights.is_contiguous() \
                or tuple(weights.shape) != (rows, k):
            raise ValueError(f"{name} must be a contiguous int32 [{rows}, {k}] tensor on the batch device")
        return C.c_void_p(weights.data_ptr())

    def rollout(self, n_rollouts: int, seed: int = 0, policy="random", prefix: Optional[torch.Tensor] = None, max_plies: int = 0,
                group: Optional[int] = None, stream=None, out: Optional[torch.Tensor] = None, return_out: Optional[torch.Tensor] = None,
                hash_out: Optional[torch.Tensor] = None, order_out: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None):
        """From the state every env is in now, play the rest of its episode n_rollouts times; the batch is left exactly as it was.
        Rollout r routes its prefix (int32 [rows, n_rollouts, stride] of 1-based net ids, <= 0 ends a list; entries that are not legal
        are skipped and flagged BAD_ACTION), then continues under `policy`: "stop" (the prefix only) or "random" (what random_actions(
        _lib.rollout_seed(seed, r)) would pick at every ply, until no net is left or max_plies real routes were made) or "weighted"
        (the same with weighted_actions(weights, ...): `weights` int32 [rows, k_max], one row per env shared by its rollouts; XR-Pick v1
        of include/xroute_hip.h, so unit weights are the random policy bit for bit).  Returns a dict
        of device tensors: `out` int32 [rows, R, 8] = {d_violation, d_wirelength, d_via, status OR, plies, nlegal_end, path_len_sum, 0},
        `ret` float64 [rows, R] (the sum of the per-step rewards), `hash` int64 [rows, R] (the env's hash chain continued) and `order`
        int32 [rows, R, k_max] (the nets routed, 0 past `plies`).  A done env holds the empty rollout.  group: an env group (rows = its
        slots, enqueued on `stream`, default the current stream); None: the whole batch."""
        if group is None:
            g, rows = -1, self.n_envs
        else:
            lo, hi = self.group_bounds(group)
            g, rows = int(group), hi - lo
        R = int(n_rollouts)
        if not 1 <= R <= _lib.XR_ROLLOUT_MAX:
            raise ValueError(f"n_rollouts must be in 1..{_lib.XR_ROLLOUT_MAX}, got {n_rollouts}")
        if rows * R >= 2 ** 31:
            raise ValueError("rows x n_rollouts does not fit 31 bits")
        pol = self._ROLLOUT_POLICY.get(policy, policy) if isinstance(policy, str) else policy
        if isinstance(pol, bool) or pol not in (_lib.XR_ROLLOUT_STOP, _lib.XR_ROLLOUT_RANDOM, _lib.XR_ROLLOUT_WEIGHTED):
            raise ValueError(f"policy must be 'stop', 'random' or 'weighted' (XR_ROLLOUT_STOP / _RANDOM / _WEIGHTED), got {policy!r}")
        if (pol == _lib.XR_ROLLOUT_WEIGHTED) != (weights is not None):
            raise ValueError(f"policy 'weighted' takes `weights`, and no other policy does: got policy {policy!r} "
                             f"{'with' if weights is not None else 'without'} weights")
        wp = self._check_weights(weights, rows) if weights is not None else None
        if int(max_plies) < 0:
            raise ValueError(f"max_plies must be >= 0, got {max_plies}")
        k = max(int(self.k_max), 1)
        bufs = {"out": (out, torch.int32, (rows, R, 8)), "return_out": (return_out, torch.float64, (rows, R)),
                "hash_out": (hash_out, torch.int64, (rows, R)), "order_out": (order_out, torch.int32, (rows, R, k))}
        if any(t is None for t, _, _ in bufs.values()):
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
                bufs = {n: (torch.empty(shp, dtype=dt, device=self.device) if t is None else t, dt, shp) for n, (t, dt, shp) in bufs.items()}
        for name, (t, dt, shp) in bufs.items():
            if t.device != self.device or t.dtype != dt or not t.is_contiguous() or tuple(t.shape) != shp:
                raise ValueError(f"{name} must be a contiguous {str(dt).replace('torch.', '')} {list(shp)} tensor on the batch device")
        pp, stride = None, 0
        if prefix is not None:
            if prefix.device != self.device or prefix.dtype != torch.int32 or not prefix.is_contiguous() or prefix.dim() != 3 \
                    or tuple(prefix.shape[:2]) != (rows, R) or prefix.shape[2] < 1:
                raise ValueError(f"prefix must be a contiguous int32 [{rows}, {R}, stride >= 1] tensor on the batch device")
            pp, stride = C.c_void_p(prefix.data_ptr()), int(prefix.shape[2])
        ptr = {n: C.c_void_p(t.data_ptr()) for n, (t, _, _) in bufs.items()}
        with torch.cuda.device(self.device):
            if wp is not None:
                _lib.check(self.L.xr_batch_rollout_weighted(self._h, g, R, int(pol), C.c_uint64(int(seed) & (2 ** 64 - 1)), pp, stride, int(max_plies),
                                                            ptr["out"], ptr["return_out"], ptr["hash_out"], ptr["order_out"], k, wp, k,
                                                            self._stream_arg(stream)))
            else:
                _lib.check(self.L.xr_batch_rollout(self._h, g, R, int(pol), C.c_uint64(int(seed) & (2 ** 64 - 1)), pp, stride, int(max_plies),
                                                   ptr["out"], ptr["return_out"], ptr["hash_out"], ptr["order_out"], k, self._stream_arg(stream)))
        return {"out": bufs["out"][0], "ret": bufs["return_out"][0], "hash": bufs["hash_out"][0], "order": bufs["order_out"][0]}

    # ---- peek: the state after a line of play, packed, without stepping (xr_batch_peek) ------------------------------------------
    def peek(self, prefix: Optional[torch.Tensor], n_lines: Optional[int] = None, max_plies: int = 0, region_base: int = 0,
             row_bytes: Optional[int] = None, group: Optional[int] = None, stream=None, rows_out: Optional[torch.Tensor] = None,
             out: Optional[torch.Tensor] = None, return_out: Optional[torch.Tensor] = None, hash_out: Optional[torch.Tensor] = None,
             order_out: Optional[torch.Tensor] = None):
        """From the state every env is in now, the state it WOULD be in after each of L lines of play; the batch is left exactly as it
        was.  Line l of a row routes prefix[row, l] (int32 [rows, L, stride] of 1-based net ids, <= 0 ends a list; entries that are not
        legal are skipped and flagged BAD_ACTION) in a throw-away copy of the slot and stops.  prefix=None needs n_lines: every line is
        the env's current state.  Returns a dict of device tensors: `rows` uint8 [rows, L, row_bytes], the packed state row after each
        line in pack_state's format (expand_state(rows.view(-1, row_bytes)) gives the head rows step_compact would write, nlegal and
        region; bytes past state_row_bytes() are not written), and `out`, `ret`, `hash`, `order` exactly as rollout(policy="stop")
        returns them for the same prefix.  row_bytes: a multiple of 8, default state_row_bytes().  group: an env group (rows = its
        slots, enqueued on `stream`, default the current stream); None: the whole batch."""
        if group is None:
            g, rows = -1, self.n_envs
        else:
            lo, hi = self.group_bounds(group)
            g, rows = int(group), hi - lo
        if prefix is None:
            if n_lines is None:
                raise ValueError("peek(prefix=None) needs n_lines")
            L = int(n_lines)
        else:
            if not isinstance(prefix, torch.Tensor) or prefix.dim() != 3:
                raise ValueError(f"prefix must be a contiguous int32 [{rows}, n_lines, stride >= 1] tensor on the batch device")
            L = int(prefix.shape[1]) if n_lines is None else int(n_lines)
        if not 1 <= L <= _lib.XR_PEEK_MAX:
            raise ValueError(f"n_lines must be in 1..{_lib.XR_PEEK_MAX}, got {L}")
        if rows * L >= 2 ** 31:
            raise ValueError("rows x n_lines does not fit 31 bits")
        if int(max_plies) < 0:
            raise ValueError(f"max_plies must be >= 0, got {max_plies}")
        pp, stride = None, 0
        if prefix is not None:
            if prefix.device != self.device or prefix.dtype != torch.int32 or not prefix.is_contiguous() \
                    or tuple(prefix.shape[:2]) != (rows, L) or prefix.shape[2] < 1:
                raise ValueError(f"prefix must be a contiguous int32 [{rows}, {L}, stride >= 1] tensor on the batch device")
            pp, stride = C.c_void_p(prefix.data_ptr()), int(prefix.shape[2])
        need = 16 + 8 * (int(self.legal_words) + (int(self.n_max) + 63) // 64)
        rb = int(row_bytes) if row_bytes is not None else (int(rows_out.shape[-1]) if isinstance(rows_out, torch.Tensor) and rows_out.dim() == 3
                                                           else need)
        if rb % 8 != 0 or rb < need:
            raise ValueError(f"row_bytes must be a multiple of 8 and >= state_row_bytes() = {need}, got {rb}")
        k = max(int(self.k_max), 1)
        bufs = {"rows_out": (rows_out, torch.uint8, (rows, L, rb)), "out": (out, torch.int32, (rows, L, 8)),
                "return_out": (return_out, torch.float64, (rows, L)), "hash_out": (hash_out, torch.int64, (rows, L)),
                "order_out": (order_out, torch.int32, (rows, L, k))}
        if any(t is None for t, _, _ in bufs.values()):
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
                bufs = {n: (torch.empty(shp, dtype=dt, device=self.device) if t is None else t, dt, shp) for n, (t, dt, shp) in bufs.items()}
        for name, (t, dt, shp) in bufs.items():
            if not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != dt or not t.is_contiguous() or tuple(t.shape) != shp:
                raise ValueError(f"{name} must be a contiguous {str(dt).replace('torch.', '')} {list(shp)} tensor on the batch device")
        if bufs["rows_out"][0].data_ptr() % 8 != 0:
            raise ValueError("rows_out must be 8-byte aligned")
        ptr = {n: C.c_void_p(t.data_ptr()) for n, (t, _, _) in bufs.items()}
        with torch.cuda.device(self.device):
            _lib.check(self.L.xr_batch_peek(self._h, g, L, pp, stride, int(max_plies), ptr["rows_out"], rb, int(region_base), ptr["out"],
                                            ptr["return_out"], ptr["hash_out"], ptr["order_out"], k, self._stream_arg(stream)))
        return {"rows": bufs["rows_out"][0], "out": bufs["out"][0], "ret": bufs["return_out"][0], "hash": bufs["hash_out"][0],
                "order": bufs["order_out"][0]}

    # ---- branch: env slots take other slots' state, on the device (xr_batch_branch) ----------------------------------------------
    def branch(self, parent: torch.Tensor, group: Optional[int] = None, stream=None) -> None:
        """Row i continues from the state row parent[i] is in now (int32 [rows] on the device; rows and indices relative to the group's
        first slot when `group` is given): every per-env array fetch() returns is copied, gather semantics — every read sees the state
        before the call, so swaps, cycles, chains and fan-outs are fine.  parent[i] < 0 or == i keeps the slot; parent[i] >= rows keeps
        it and flags BAD_ACTION in its status.  Nothing leaves the device and nothing synchronises.  A slot may now play another region:
        region_epoch is bumped."""
        if group is None:
            g, rows = -1, self.n_envs
        else:
            lo, hi = self.group_bounds(group)
            g, rows = int(group), hi - lo
        if not isinstance(parent, torch.Tensor) or parent.device != self.device or parent.dtype != torch.int32 or not parent.is_contiguous() \
                or tuple(parent.shape) != (rows,):
            raise ValueError(f"parent must be a contiguous int32 [{rows}] tensor on the batch device")
        with torch.cuda.device(self.device):
            _lib.check(self.L.xr_batch_branch(self._h, g, C.c_void_p(parent.data_ptr()), self._stream_arg(stream)))
        self.region_epoch += 1

    # ---- tree search: MCTS over net orderings, the tree on the device (xr_batch_tree_search) ------------------------------------------
    def tree_search(self, n_waves: int, n_par: int, seed: int = 0, prior: Optional[torch.Tensor] = None, node_cap: Optional[int] = None,
                    c_init: float = 1.25, c_base: float = 19652.0, group: Optional[int] = None, stream=None, trace: bool = False,
                    sim_weights: Optional[torch.Tensor] = None, keep: bool = False, played: Optional[torch.Tensor] = None):
        """XR-Tree v1 (include/xroute_hip.h) from the state every env is in now: n_waves waves of n_par simulations per row, each a pUCT
        descent of the row's tree, a random rollout below the selected node and a backup — one enqueue-only call; the batch is left
        exactly as it was.  prior: None (uniform) or float32 [rows, k_max] weights per net (not finite or < 0 counts as 0; softmax is the
        caller's business).  node_cap: nodes per row, default 1 + n_waves * n_par * k_max (1 + (n_waves * n_par + 1) * k_max always suffices).  Returns a dict of device
        tensors: `visits` int32 [rows, k_max] (N of the root's child of net n at n - 1), `value` float64 [rows, k_max] (W / N, -inf
        where N == 0), `info` int32 [rows, 4] = {simulations, nodes_used, max_depth, flags (XR_TREE_POOL_FULL)}, `best_order` int32
        [rows, k_max] and `best_return` float64 [rows] (the best line any simulation saw); with trace=True also `paths` int32 [rows,
        n_waves * n_par, k_max] and `returns` float64 [rows, n_waves * n_par], every simulation in (wave, lane) order.  A done env holds
        the empty result.  group: an env group (rows = its slots, enqueued on `stream`); None: the whole batch.  sim_weights: None, or
        int32 [rows, k_max]: the simulations below a selected node follow rollout(policy="weighted", weights=sim_weights) instead of the
        random policy (xr_batch_tree_search_weighted).  keep=True: the search of "XR-Tree v1, kept" (xr_batch_tree_search_keep), on the
        caller's kept-tree pool: it leaves its tree behind, and continues from the tree the caller's last kept call left where `played`
        says how the env has moved since — None: every row starts over; int32 [rows]: 0 the env has not moved, a > 0 the env has made
        exactly one step, of net a; a row whose key does not agree (and any negative entry) starts over.  The dict then also holds
        `kept` int32 [rows, 2] = {visits of the new root carried in, nodes carried}, and `info`'s flags carry XR_TREE_KEPT.  node_cap
        is part of the pool's shape (a call with another one starts every row over); its default is 1 + 4 * n_waves * n_par * k_max for
        a kept call, room for what a tree carries along."""
        if played is not None and not keep:
            raise ValueError("played needs keep=True")
        if group is None:
            g, rows = -1, self.n_envs
        else:
            lo, hi = self.group_bounds(group)
            g, rows = int(group), hi - lo
        W, P = int(n_waves), int(n_par)
        if W < 1:
            raise ValueError(f"n_waves must be >= 1, got {n_waves}")
        if not 1 <= P <= _lib.XR_ROLLOUT_MAX:
            raise ValueError(f"n_par must be in 1..{_lib.XR_ROLLOUT_MAX}, got {n_par}")
        if W * P > _lib.XR_TREE_MAX_SIMS:
            raise ValueError(f"n_waves x n_par must be <= {_lib.XR_TREE_MAX_SIMS}, got {W * P}")
        ci, cb = float(c_init), float(c_base)
        if not math.isfinite(ci):
            raise ValueError(f"c_init must be finite, got {c_init}")
        if not (math.isfinite(cb) and cb > 0):
            raise ValueError(f"c_base must be finite and > 0, got {c_base}")
        k = max(int(self.k_max), 1)
        cap = 1 + (4 if keep else 1) * W * P * k if node_cap is None else int(node_cap)
        if not 1 <= cap < 2 ** 31:
            raise ValueError(f"node_cap must be in 1..2^31 - 1, got {node_cap}")
        pp = None
        if prior is not None:
            if not isinstance(prior, torch.Tensor) or prior.device != self.device or prior.dtype != torch.float32 or not prior.is_contiguous() \
                    or tuple(prior.shape) != (rows, k):
                raise ValueError(f"prior must be a contiguous float32 [{rows}, {k}] tensor on the batch device")
            pp = C.c_void_p(prior.data_ptr())
        wp = self._check_weights(sim_weights, rows, "sim_weights") if sim_weights is not None else None
        pl = None
        if played is not None:
            if not isinstance(played, torch.Tensor) or played.device != self.device or played.dtype != torch.int32 or not played.is_contiguous() \
                    or tuple(played.shape) != (rows,):
                raise ValueError(f"played must be a contiguous int32 [{rows}] tensor on the batch device")
            pl = C.c_void_p(played.data_ptr())
        shapes = {"visits": (torch.int32, (rows, k)), "value": (torch.float64, (rows, k)), "info": (torch.int32, (rows, 4)),
                  "best_order": (torch.int32, (rows, k)), "best_return": (torch.float64, (rows,))}
        if trace:
            shapes.update(paths=(torch.int32, (rows, W * P, k)), returns=(torch.float64, (rows, W * P)))
        if keep:
            shapes.update(kept=(torch.int32, (rows, 2)))
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
            res = {n: torch.empty(shp, dtype=dt, device=self.device) for n, (dt, shp) in shapes.items()}
        ptr = {n: C.c_void_p(t.data_ptr()) for n, t in res.items()}
        with torch.cuda.device(self.device):
            if keep:
                _lib.check(self.L.xr_batch_tree_search_keep(self._h, g, pl, W, P, C.c_uint64(int(seed) & (2 ** 64 - 1)), pp, cap, ci, cb, ptr["visits"],
                                                            ptr["value"], k, ptr["info"], ptr["best_order"], ptr["best_return"], ptr.get("paths"),
                                                            ptr.get("returns"), wp, ptr["kept"], self._stream_arg(stream)))
            elif wp is not None:
                _lib.check(self.L.xr_batch_tree_search_weighted(self._h, g, W, P, C.c_uint64(int(seed) & (2 ** 64 - 1)), pp, cap, ci, cb, ptr["visits"],
                                                                ptr["value"], k, ptr["info"], ptr["best_order"], ptr["best_return"],
                                                                ptr.get("paths"), ptr.get("returns"), wp, self._stream_arg(stream)))
            else:
                _lib.check(self.L.xr_batch_tree_search(self._h, g, W, P, C.c_uint64(int(seed) & (2 ** 64 - 1)), pp, cap, ci, cb, ptr["visits"],
                                                       ptr["value"], k, ptr["info"], ptr["best_order"], ptr["best_return"], ptr.get("paths"),
                                                       ptr.get("returns"), self._stream_arg(stream)))
        return res

    # ---- evaluated tree search: leaves valued by the caller's network (xr_batch_tree_open / _leaves / _backup) -------------------------
    def _tree_rows(self, group):
        if group is None:
            return -1, self.n_envs
        lo, hi = self.group_bounds(group)
        return int(group), hi - lo

    def _tree_tensor(self, t, name: str, dtype, shape):
        if not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} must be a contiguous {str(dtype).replace('torch.', '')} {list(shape)} tensor on the batch device")
        return C.c_void_p(t.data_ptr())

    def tree_open(self, n_par: int, max_sims: int, root_prior: Optional[torch.Tensor] = None, node_cap: Optional[int] = None,
                  c_init: float = 1.25, c_base: float = 19652.0, group: Optional[int] = None, stream=None, keep: bool = False,
                  played: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """Start a session of "XR-Tree v2, evaluated" (include/xroute_hip.h) from the state every env is in now: a tree per row whose
        simulations stop at the selected leaf; tree_leaves() hands out a wave's leaves as packed state rows, the caller's evaluator values
        them, tree_backup() takes the values.  n_par: lanes per wave (1..XR_PEEK_MAX); max_sims: the simulations the session may run
        (n_par..XR_TREE_MAX_SIMS); root_prior: None (uniform) or float32 [rows, k_max] weights per net, the prior of every block the
        search expands until an evaluator's leaf prior replaces it; node_cap: nodes per row, default 1 + (max_sims + 1) * k_max (always
        enough).  The env's legal set is copied: a caller who steps the env before the last tree_backup must open again.  Enqueue-only;
        the batch is left exactly as it was.  group: an env group (rows = its slots, enqueued on `stream`); None: the whole batch.
        keep=True: the session of "XR-Tree v2, kept" (xr_batch_tree_reopen): it is keyed to the state it starts from, and continues from
        the tree the caller's last keyed session left where `played` says how the env has moved since — None: every row starts over;
        int32 [rows]: 0 the env has not moved, a > 0 the env has made exactly one step, of net a; a row whose key does not agree (and any
        negative entry) starts over.  max_sims then bounds this session's simulations.  Returns `kept` int32 [rows, 2] = {visits of the
        new root carried in, nodes carried} (None without keep); info's flags carry XR_TREE_KEPT.  node_cap is part of the pool's shape
        (a reopen with another one starts every row over); its default with keep is 1 + 4 * (max_sims + 1) * k_max, room for what a
        tree carries along."""
        if played is not None and not keep:
            raise ValueError("played needs keep=True")
        g, rows = self._tree_rows(group)
        P, M = int(n_par), int(max_sims)
        if not 1 <= P <= _lib.XR_PEEK_MAX:
            raise ValueError(f"n_par must be in 1..{_lib.XR_PEEK_MAX}, got {n_par}")
        if not P <= M <= _lib.XR_TREE_MAX_SIMS:
            raise ValueError(f"max_sims must be in n_par..{_lib.XR_TREE_MAX_SIMS}, got {max_sims}")
        if rows * P >= 2 ** 31:
            raise ValueError("rows x n_par does not fit 31 bits")
        ci, cb = float(c_init), float(c_base)
        if not math.isfinite(ci):
            raise ValueError(f"c_init must be finite, got {c_init}")
        if not (math.isfinite(cb) and cb > 0):
            raise ValueError(f"c_base must be finite and > 0, got {c_base}")
        k = max(int(self.k_max), 1)
        cap = 1 + (4 if keep else 1) * (M + 1) * k if node_cap is None else int(node_cap)
        if not 1 <= cap < 2 ** 31:
            raise ValueError(f"node_cap must be in 1..2^31 - 1, got {node_cap}")
        pp = self._tree_tensor(root_prior, "root_prior", torch.float32, (rows, k)) if root_prior is not None else None
        pl = self._tree_tensor(played, "played", torch.int32, (rows,)) if played is not None else None
        kept = None
        if keep:
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
                kept = torch.empty((rows, 2), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            if keep:
                _lib.check(self.L.xr_batch_tree_reopen(self._h, g, pl, P, cap, ci, cb, M, pp, k, C.c_void_p(kept.data_ptr()), self._stream_arg(stream)))
            else:
                _lib.check(self.L.xr_batch_tree_open(self._h, g, P, cap, ci, cb, M, pp, k, self._stream_arg(stream)))
        if not hasattr(self, "_tree_sessions"):
            self._tree_sessions = {}
        self._tree_sessions[g] = P
        return kept

    def _tree_session(self, group, fn: str):
        g, rows = self._tree_rows(group)
        P = getattr(self, "_tree_sessions", {}).get(g)
        if P is None:
            raise _lib.XRouteError(_lib.XR_ERR_STATE, f"{fn}: no open session of this caller (tree_open first)")
        return g, rows, P

    def tree_leaves(self, region_base: int = 0, row_bytes: Optional[int] = None, group: Optional[int] = None, stream=None,
                    rows_out: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, return_out: Optional[torch.Tensor] = None,
                    paths_out: Optional[torch.Tensor] = None, leaf_out: Optional[torch.Tensor] = None):
        """One wave of the open session: n_par pUCT descents per row (XR-Tree v1's Select), then one peek launch along the paths.  Returns a
        dict of device tensors: `rows` uint8 [rows, n_par, row_bytes], `out` int32 [rows, n_par, 8] and `ret` float64 [rows, n_par] —
        exactly what peek(paths) returns — `paths` int32 [rows, n_par, k_max] (each ended by 0) and `leaf` int32 [rows, n_par, 2] =
        {node, flags: XR_TREE_LEAF_TERMINAL | XR_TREE_LEAF_FRESH | XR_TREE_LEAF_NONE}.  Every wave is followed by tree_backup()."""
        g, rows, P = self._tree_session(group, "tree_leaves")
        need = 16 + 8 * (int(self.legal_words) + (int(self.n_max) + 63) // 64)
        rb = int(row_bytes) if row_bytes is not None else (int(rows_out.shape[-1]) if isinstance(rows_out, torch.Tensor) and rows_out.dim() == 3
                                                           else need)
        if rb % 8 != 0 or rb < need:
            raise ValueError(f"row_bytes must be a multiple of 8 and >= state_row_bytes() = {need}, got {rb}")
        k = max(int(self.k_max), 1)
        bufs = {"rows_out": (rows_out, torch.uint8, (rows, P, rb)), "out": (out, torch.int32, (rows, P, 8)),
                "return_out": (return_out, torch.float64, (rows, P)), "paths_out": (paths_out, torch.int32, (rows, P, k)),
                "leaf_out": (leaf_out, torch.int32, (rows, P, 2))}
        for n, (t, dt, shp) in bufs.items():          # the caller's buffers first: a bad one is refused before anything is allocated
            if t is not None:
                self._tree_tensor(t, n, dt, shp)
        if any(t is None for t, _, _ in bufs.values()):
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
                bufs = {n: (torch.empty(shp, dtype=dt, device=self.device) if t is None else t, dt, shp) for n, (t, dt, shp) in bufs.items()}
        ptr = {n: self._tree_tensor(t, n, dt, shp) for n, (t, dt, shp) in bufs.items()}
        if bufs["rows_out"][0].data_ptr() % 8 != 0:
            raise ValueError("rows_out must be 8-byte aligned")
        with torch.cuda.device(self.device):
            _lib.check(self.L.xr_batch_tree_leaves(self._h, g, ptr["rows_out"], rb, int(region_base), ptr["out"], ptr["return_out"], ptr["paths_out"],
                                                   ptr["leaf_out"], self._stream_arg(stream)))
        return {"rows": bufs["rows_out"][0], "out": bufs["out"][0], "ret": bufs["return_out"][0], "paths": bufs["paths_out"][0],
                "leaf": bufs["leaf_out"][0]}

    def tree_backup(self, value: torch.Tensor, leaf_prior: Optional[torch.Tensor] = None, group: Optional[int] = None, stream=None):
        """The evaluator's answer to the last tree_leaves(): value float64 [rows, n_par] (the return expected from each leaf's state to the
        end of its episode; not finite counts as 0, a terminal leaf's is not read) and leaf_prior None or float32 [rows, n_par, k_max]
        (weights over the children of each lane's leaf; applied to leaves that lane has just expanded).  Returns a dict of device tensors
        as tree_search() does — `visits`, `value`, `info` = {simulations so far, nodes_used, max_depth, flags}, `best_order`,
        `best_return` (from terminal simulations only) — and `returns` float64 [rows, n_par], the wave's G."""
        g, rows, P = self._tree_session(group, "tree_backup")
        k = max(int(self.k_max), 1)
        vp = self._tree_tensor(value, "value", torch.float64, (rows, P))
        lp = self._tree_tensor(leaf_prior, "leaf_prior", torch.float32, (rows, P, k)) if leaf_prior is not None else None
        shapes = {"visits": (torch.int32, (rows, k)), "value": (torch.float64, (rows, k)), "info": (torch.int32, (rows, 4)),
                  "best_order": (torch.int32, (rows, k)), "best_return": (torch.float64, (rows,)), "returns": (torch.float64, (rows, P))}
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
            res = {n: torch.empty(shp, dtype=dt, device=self.device) for n, (dt, shp) in shapes.items()}
        ptr = {n: C.c_void_p(t.data_ptr()) for n, t in res.items()}
        with torch.cuda.device(self.device):
            _lib.check(self.L.xr_batch_tree_backup(self._h, g, vp, lp, ptr["visits"], ptr["value"], ptr["info"], ptr["best_order"], ptr["best_return"],
                                                   ptr["returns"], self._stream_arg(stream)))
        return res

    def alloc_head(self) -> torch.Tensor:
        """[n_envs, 2*n_max] fp32 buffer for the compact-consumer step (planes 0..1 of every env)."""
        return torch.empty((self.n_envs, 2 * self.n_max), dtype=torch.float32, device=self.device)

    def step_compact(self, actions: torch.Tensor, head_out: torch.Tensor):
        """Game.step for every env + only the two observation planes that change (obstacles, net order):
        xr_batch_step_compact.  The net planes come once per (region, net) from `net_planes`."""
        if actions.device != self.device or actions.dtype != torch.int32 or not actions.is_contiguous() \
                or actions.numel() != self.n_envs:
            raise ValueError("actions must be a contiguous int32 tensor of n_envs entries on the batch device")
        if head_out.device != self.device or head_out.dtype != torch.float32 or not head_out.is_contiguous() \
                or head_out.dim() != 2 or head_out.shape[0] < self.n_envs:
            raise ValueError("head_out must be a contiguous fp32 [n_envs, stride] tensor on the batch device")
        with torch.cuda.device(self.device):
            _lib.check(self.L.xr_batch_step_compact(self._h, C.c_void_p(actions.data_ptr()), C.c_void_p(head_out.data_ptr()),
                                                    head_out.shape[1], _stream_ptr(self.device)))
        return head_out

    def net_planes(self, region: torch.Tensor, net: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The 7 static planes of (region index, 1-based net id) pairs: [n, 7*n_max] fp32 (xr_batch_net_planes)."""
        region = region.to(device=self.device, dtype=torch.int32).contiguous()
        net = net.to(device=self.device, dtype=torch.int32).contiguous()
        n = region.numel()
        if net.numel() != n:
            raise ValueError("region and net must have the same length")
        if out is None:
            out = torch.empty((n, 7 * self.n_max), dtype=torch.float32, device=self.device)
        if out.device != self.device or out.dtype != torch.float32 or not out.is_contiguous() or out.dim() != 2 or out.shape[0] < n:
            raise ValueError("out must be a contiguous fp32 [n, stride] tensor on the batch device")
        with torch.cuda.device(self.device):
            _lib.check(self.L.xr_batch_net_planes(self._h, C.c_void_p(region.data_ptr()), C.c_void_p(net.data_ptr()), n,
                                                  C.c_void_p(out.data_ptr()), out.shape[1], _stream_ptr(self.device)))
        return out

    # ---- compact state for a central learner (gather compact state, expand on the learner GPU) ----------------
    def state_row_bytes(self) -> int:
        """Bytes of one packed state row of this batch (region, nets left, legal bitmask, one occupancy bit per node)."""
        n = C.c_int64()
        _lib.check(self.L.xr_batch_state_row_bytes(self._h, C.byref(n)))
        return int(n.value)

    def pack_state(self, out: Optional[torch.Tensor] = None, region_base: int = 0, row_bytes: Optional[int] = None) -> torch.Tensor:
        """One packed row per env slot (uint8 [n_envs, row_bytes]): what planes 0..1 of its observation are functions of — ready for
        ONE all_gather to a learner.  `region_base` turns the local region index into an index of the learner's region table."""
        rb = int(row_bytes) if row_bytes is not None else (int(out.shape[1]) if out is not None else self.state_row_bytes())
        if out is None:
            out = torch.empty((self.n_envs, rb), dtype=torch.uint8, device=self.device)
        if out.dtype != torch.uint8 or not out.is_contiguous() or tuple(out.shape) != (self.n_envs, rb):
            raise ValueError("out must be a contiguous uint8 [n_envs, row_bytes] tensor")
        with torch.cuda.device(self.device):
            _lib.check(self.L.xr_batch_pack_state(self._h, C.c_void_p(out.data_ptr()), rb, int(region_base), _stream_ptr(self.device)))
        return out

    def ingest_state(self, owner: torch.Tensor, legal: torch.Tensor, cum: torch.Tensor):
        """Adopt a new state of every env slot produced by an EXTERNAL simulator (the client half of the reference's Game.step without the
        route, baseline/baseline_utils.py:420-438 — BASELINE config 2): owner int16 [n_envs, n_max], legal int64 / uint64 [n_envs, legal_words],
        cum int32 [n_envs, 3].  The records then carry the metric deltas, the reward and `done`; `observation()` builds the grid."""
        if owner.dtype != torch.int16 or tuple(owner.shape) != (self.n_envs, self.n_max) or not owner.is_contiguous():
            raise ValueError("owner must be a contiguous int16 [n_envs, n_max] tensor")
        if legal.dtype not in (torch.int64, torch.uint64) or tuple(legal.shape) != (self.n_envs, self.legal_words) or not legal.is_contiguous():
            raise ValueError("legal must be a contiguous 64-bit [n_envs, legal_words] tensor")
        if cum.dtype != torch.int32 or tuple(cum.shape) != (self.n_envs, 3) or not cum.is_contiguous():
            raise ValueError("cum must be a contiguous int32 [n_envs, 3] tensor")
        with torch.cuda.device(self.device):
            _lib.check(self.L.xr_batch_ingest_state(self._h, C.c_void_p(owner.data_ptr()), C.c_void_p(legal.data_ptr()), C.c_void_p(cum.data_ptr()),
                                                    _stream_ptr(self.device)))

    def expand_state(self, rows: torch.Tensor, head_out: Optional[torch.Tensor] = None, nlegal_out: Optional[torch.Tensor] = None,
                     region_out: Optional[torch.Tensor] = None):
        """Learner side: packed rows (uint8 [n, row_bytes], e.g. the all_gather of every rank's `pack_state`) -> (head [n, stride] fp32 with
        planes 0..1 of every env exactly as `step_compact` writes them, nlegal int32 [n], region int32 [n]).  This batch supplies the
        region table (it must hold every region the rows name); rows that do not parse are flagged nlegal = region = -1."""
        if rows.dtype != torch.uint8 or rows.dim() != 2 or not rows.is_contiguous():
            raise ValueError("rows must be a contiguous uint8 [n, row_bytes] tensor")
        n = int(rows.shape[0])
        if head_out is None:
            head_out = torch.empty((n, 2 * self.n_max), dtype=torch.float32, device=self.device)
        if nlegal_out is None:
            nlegal_out = torch.empty(n, dtype=torch.int32, device=self.device)
        if region_out is None:
            region_out = torch.empty(n, dtype=torch.int32, device=self.device)
        if head_out.dtype != torch.float32 or head_out.shape[0] != n or head_out.stride(1) != 1:
            raise ValueError("head_out must be fp32 [n, stride] with unit inner stride")
        with torch.cuda.device(self.device):
            _lib.check(self.L.xr_batch_expand_state(self._h, C.c_void_p(rows.data_ptr()), int(rows.shape[1]), n, C.c_void_p(head_out.data_ptr()),
                                                    int(head_out.stride(0)), C.c_void_p(nlegal_out.data_ptr()), C.c_void_p(region_out.data_ptr()),
                                                    _stream_ptr(self.device)))
        return head_out, nlegal_out, region_out

    def route_occupancy(self):
        """(resident workgroups per CU, LDS bytes per workgroup) of the step kernel for the loaded regions."""
        n, lds = C.c_int32(0), C.c_int64(0)
        _lib.check(self.L.xr_batch_route_occupancy(self._h, C.byref(n), C.byref(lds)))
        return int(n.value), int(lds.value)

    def observe_timing(self):
        """(mode, writer_ms) of the last step(actions, obs_out): mode 1 = fused launch, 2 = split (route kernel and
        net-plane writer running concurrently); writer_ms = HIP-event duration of the writer kernel (0 when fused)."""
        mode, ms = C.c_int32(0), C.c_float(0.0)
        _lib.check(self.L.xr_batch_observe_timing(self._h, C.byref(mode), C.byref(ms)))
        return int(mode.value) & ~32, float(ms.value)       # (form | 16 when the in-place path ran; bit 5: see observe_info)

    def observe_info(self) -> dict:
        """The last step(actions, obs_out) in words: form (1 fused, 2 split, 3 queue), whether the in-place path ran, and
        whether the auto router ran the line-segment sweeps in that launch (full rewrite of a batch of >= 4096 slots)."""
        mode, ms = C.c_int32(0), C.c_float(0.0)
        _lib.check(self.L.xr_batch_observe_timing(self._h, C.byref(mode), C.byref(ms)))
        m = int(mode.value)
        return {"form": m & 15, "inplace": bool(m & 16), "sweeps": bool(m & 32), "writer_ms": float(ms.value)}

    def route_order(self, orders: torch.Tensor, net_stats: Optional[torch.Tensor] = None):
        """Whole-order re-route (xr_batch_route_order): every env restarts its region and routes
        orders[e, :] (int32 [B, stride >= k_max], 1-based ids, 0-terminated) in that order, one launch.
        net_stats: optional int32 [B, stride, 4] (per net: d_vio, d_wl, d_via, route counter)."""
        if orders.device != self.device or orders.dtype != torch.int32 or not orders.is_contiguous() \
                or orders.dim() != 2 or orders.shape[0] != self.n_envs:
            raise ValueError("orders must be a contiguous int32 [n_envs, stride] tensor on the batch device")
        sp = None
        if net_stats is not None:
            if net_stats.device != self.device or net_stats.dtype != torch.int32 or not net_stats.is_contiguous() \
                    or tuple(net_stats.shape) != (self.n_envs, orders.shape[1], 4):
                raise ValueError("net_stats must be a contiguous int32 [n_envs, stride, 4] tensor on the batch device")
            sp = C.c_void_p(net_stats.data_ptr())
        with torch.cuda.device(self.device):
            _lib.check(self.L.xr_batch_route_order(self._h, C.c_void_p(orders.data_ptr()), int(orders.shape[1]), sp,
                                                   _stream_ptr(self.device)))
        return net_stats

    def random_actions(self, seed: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        if out is None:
            out = torch.empty(self.n_envs, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.L.xr_batch_random_actions(self._h, C.c_void_p(out.data_ptr()),
                                                      C.c_uint64(seed & (2 ** 64 - 1)), _stream_ptr(self.device)))
        return out

    @property
    def obs_env_stride_u8(self) -> int:
        """Recommended row stride (bytes) of a uint8 observation buffer: (2+7*k_max)*n_max rounded up to 128 bytes."""
        return ((2 + 7 * self.k_max) * self.n_max + 127) & ~127

    def alloc_observation(self, n_envs: Optional[int] = None, env_stride: Optional[int] = None, dtype=torch.float32) -> torch.Tensor:
        """[n_envs, stride] observation buffer: fp32 (stride in floats, obs_env_stride) or uint8 (stride in bytes, obs_env_stride_u8)."""
        if dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"observation dtype must be torch.float32 or torch.uint8, not {dtype}")
        n = self.n_envs if n_envs is None else n_envs
        default = self.obs_env_stride if dtype == torch.float32 else self.obs_env_stride_u8
        stride = default if env_stride is None else env_stride
        return torch.empty((n, stride), dtype=dtype, device=self.device)

    def _check_obs(self, out: torch.Tensor, rows: int, what: str):
        if out.device != self.device or out.dtype not in (torch.float32, torch.uint8) or not out.is_contiguous() or out.dim() != 2 \
                or out.shape[0] < rows:
            raise ValueError(f"{what} must be a contiguous fp32 or uint8 [{'n_envs' if rows == self.n_envs else 'rows'}, stride] tensor "
                             "on the batch device")

    def observation(self, out: Optional[torch.Tensor] = None, env_lo: int = 0, env_hi: Optional[int] = None):
        """build_3Dgrid of the current state of envs [env_lo, env_hi) into `out` ([n, stride] fp32, or uint8: the same values as
        bytes, xr_batch_observation_u8).  Env i's observation is out[i, :(2+7K_i)*N_i] viewed as [2+7K_i, Z, Y, X]."""
        env_hi = self.n_envs if env_hi is None else env_hi
        if out is None:
            out = self.alloc_observation(env_hi - env_lo)
        self._check_obs(out, env_hi - env_lo, "out")
        fn = self.L.xr_batch_observation_u8 if out.dtype == torch.uint8 else self.L.xr_batch_observation
        with torch.cuda.device(self.device):
            _lib.check(fn(self._h, C.c_void_p(out.data_ptr()), out.shape[1], env_lo, env_hi, _stream_ptr(self.device)))
        return out

    def env_observation(self, e: int, nlegal: Optional[int] = None) -> torch.Tensor:
        """Reference-shaped [1, 2+7K, Z, Y, X] observation of one env (device tensor)."""
        if nlegal is None:
            nlegal = int(self.fetch("nlegal")[e].item())
        reg = self.regions[int(self.fetch("region")[e].item())]
        X, Y, Z = reg.dims
        buf = self.observation(env_lo=e, env_hi=e + 1)
        c = 2 + 7 * nlegal
        return buf[0, : c * reg.n_nodes].view(1, c, Z, Y, X)

    # ------------------------------------------------------------------------------------------
    _FETCH = {
        "cum": (_lib.XR_FETCH_CUM, torch.int32, lambda s: (s.n_envs, 3)),
        "delta": (_lib.XR_FETCH_DELTA, torch.int32, lambda s: (s.n_envs, 3)),
        "reward": (_lib.XR_FETCH_REWARD, torch.float64, lambda s: (s.n_envs,)),
        "done": (_lib.XR_FETCH_DONE, torch.uint8, lambda s: (s.n_envs,)),
        "nlegal": (_lib.XR_FETCH_NLEGAL, torch.int32, lambda s: (s.n_envs,)),
        "status": (_lib.XR_FETCH_STATUS, torch.int32, lambda s: (s.n_envs,)),
        "legal": (_lib.XR_FETCH_LEGAL, torch.int64, lambda s: (s.n_envs, s.legal_words)),
        "path_len": (_lib.XR_FETCH_PATH_LEN, torch.int32, lambda s: (s.n_envs,)),
        "path": (_lib.XR_FETCH_PATH, torch.int32, lambda s: (s.n_envs, s.path_cap)),
        "owner": (_lib.XR_FETCH_OWNER, torch.int16, lambda s: (s.n_envs, s.n_max)),
        "hash": (_lib.XR_FETCH_HASH, torch.int64, lambda s: (s.n_envs,)),
        "region": (_lib.XR_FETCH_REGION, torch.int32, lambda s: (s.n_envs,)),
        "steps": (_lib.XR_FETCH_STEPS, torch.int64, lambda s: (1,)),
        "sweeps": (_lib.XR_FETCH_SWEEPS, torch.int32, lambda s: (s.n_envs,)),
        "phases": (_lib.XR_FETCH_PHASES, torch.int64, lambda s: (s.n_envs, 8)),
        "units": (_lib.XR_FETCH_UNITS, torch.int32, lambda s: (1,)),
        "route_order": (_lib.XR_FETCH_ROUTE_ORDER, torch.int32, lambda s: (s.n_envs,)),
        "touched": (_lib.XR_FETCH_TOUCHED, torch.int32, lambda s: (s.n_envs,)),
        "record": (_lib.XR_FETCH_RECORD, torch.uint8, lambda s: (s.n_envs, _lib.RECORD_BYTES)),
        "replay": (_lib.XR_FETCH_REPLAY, torch.int32, lambda s: (s.n_envs,)),
        "env_steps": (_lib.XR_FETCH_ENV_STEPS, torch.int64, lambda s: (s.n_envs,)),
    }
    # the arrays that ARE the env state (xr_batch_store accepts exactly these)
    # (restore order: `region` first — xr_batch_store checks legal bits and nets-left counts against the region each slot plays)
    _STATE = ("region", "owner", "legal", "nlegal", "cum", "delta", "reward", "done", "status", "path_len", "hash", "replay",
              "env_steps", "record", "steps")

    def fetch(self, what: str, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Copy one result array into a device tensor (async on the current stream)."""
        sel, dtype, shape = self._FETCH[what]
        if out is None:
            out = torch.empty(shape(self), dtype=dtype, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.L.xr_batch_fetch(self._h, sel, C.c_void_p(out.data_ptr()),
                                             out.numel() * out.element_size(), _stream_ptr(self.device)))
        return out

    def fetch_host(self, what: str, out: torch.Tensor) -> torch.Tensor:
        """Copy one result array straight into a PINNED host tensor (async on the current stream; synchronise the stream
        before reading it).  One transfer instead of device copy + .cpu(): the small-batch path."""
        sel, dtype, shape = self._FETCH[what]
        if out.device.type != "cpu" or not out.is_pinned() or out.dtype != dtype or not out.is_contiguous():
            raise ValueError("out must be a contiguous pinned host tensor of the array's dtype")
        with torch.cuda.device(self.device):
            _lib.check(self.L.xr_batch_fetch(self._h, sel, C.c_void_p(out.data_ptr()),
                                             out.numel() * out.element_size(), _stream_ptr(self.device)))
        return out

    def state_dict(self) -> dict:
        """Env checkpoint: every array that is state of the env slots, as CPU tensors (+ the sizes a restore must match).  The
        reference never checkpoints its env — the state lives in the simulator process; only its agents are saved
        (baseline/DQN/DQN.py:236-242)."""
        d = {k: self.fetch(k).cpu() for k in self._STATE}
        d["_meta"] = torch.tensor([self.n_envs, self.n_regions, self.n_max, self.legal_words], dtype=torch.int64)
        d["_fingerprint"] = torch.from_numpy(np.frombuffer(self.fingerprint(), np.uint8).copy())
        return d

    def fingerprint(self) -> bytes:
        """sha256 over what the env state is a state OF: every region's content (dims, tracks, layer directions, node records, initial
        metrics, guide boxes) and the config fields that change what a step computes (costs, rotation period, XR-Maze v2 knobs)."""
        import hashlib
        h = hashlib.sha256()
        c = self.cfg
        h.update(np.array([c.via_cost, c.drc_cost, c.drc_unit, c.max_route_count, c.guide_cost, c.guide_margin, c.maze_end_iter,
                           len(self.regions)], np.int64).tobytes())
        for r in self.regions:
            h.update(np.array([*r.dims, r.n_nets, *[int(v) for v in r.metrics0]], np.int64).tobytes())
            for a, dt in ((r.xs, np.int32), (r.ys, np.int32), (r.layer_dir, np.uint8), (r.nodes, np.uint32)):
                h.update(np.ascontiguousarray(a, dt).tobytes())
            if getattr(r, "guide_off", None) is not None:
                h.update(np.ascontiguousarray(r.guide_off, np.int32).tobytes())
                h.update(np.ascontiguousarray(r.guide_box, np.int16).tobytes())
        return h.digest()

    def load_state_dict(self, d: dict, host_checks: bool = True):
        """Restore a state_dict() into a batch created with the same regions and config: it continues bit-identically.
        All-or-nothing: a dict that is refused — here on the host, or by xr_batch_store (`host_checks=False` leaves the range checks to
        the library: the rollback path) — leaves the batch in the state it had."""
        meta = [int(v) for v in d["_meta"]]
        if meta != [self.n_envs, self.n_regions, self.n_max, self.legal_words]:
            raise ValueError(f"state of a different batch: (n_envs, n_regions, n_max, legal_words) = {meta}")
        if "_fingerprint" in d and bytes(d["_fingerprint"].numpy().tobytes()) != self.fingerprint():
            raise ValueError("state of a different batch: the regions or the step-relevant config (costs, rotation, XR-Maze v2 knobs) differ")
        #  nothing is stored until EVERYTHING has been checked: shapes of all arrays, then on the host what xr_batch_store would
        # refuse later (a region index out of range, legal bits beyond the region's nets, a nets-left count that is not the popcount) — and
        # should a store fail all the same, the batch is rolled back to the state it had, so a caller never holds a half-restored batch.
        optional = ("steps",)                  # a dump written before `steps` was part of the state keeps the batch's own counter
        missing = [k for k in self._STATE if k not in d and k not in optional]
        if missing:
            raise ValueError(f"state dict lacks {missing} (written by an older version of RegionBatch.state_dict?)")
        staged = {}
        for k in self._STATE:
            if k not in d:
                continue
            sel, dtype, shape = self._FETCH[k]
            t = torch.as_tensor(d[k]).to(dtype=dtype).contiguous()
            if tuple(t.shape) != tuple(shape(self)):
                raise ValueError(f"state array {k}: shape {tuple(t.shape)} != {tuple(shape(self))}")
            staged[k] = t
        if host_checks:
            self._check_state_ranges(staged)
        backup = {k: self.fetch(k) for k in staged}
        self.region_epoch += 1
        with torch.cuda.device(self.device):
            try:
                self._store_arrays({k: t.to(self.device) for k, t in staged.items()})
            except Exception:
                self._store_arrays(backup)
                raise

    def _check_state_ranges(self, staged: dict):
        """What xr_batch_store range-checks (csrc/xr_batch.cpp), on the host and BEFORE anything is stored; same error convention."""
        reg = staged["region"].cpu().numpy().astype(np.int64)
        if reg.size and (reg.min() < 0 or reg.max() >= self.n_regions):
            raise _lib.XRouteError(_lib.XR_ERR_RANGE, "state array region: index outside the batch's regions")
        words = staged["legal"].cpu().numpy().view(np.uint64).reshape(self.n_envs, self.legal_words)
        nn = np.array([int(r.n_nets) for r in self.regions], np.int64)[reg]
        bit0 = np.arange(self.legal_words, dtype=np.int64)[None, :] * 64
        nbits = np.clip(nn[:, None] - bit0, 0, 64)
        allowed = np.where(nbits >= 64, np.uint64(0xFFFFFFFFFFFFFFFF), (np.uint64(1) << nbits.astype(np.uint64)) - np.uint64(1))
        if np.any(words & ~allowed):
            raise _lib.XRouteError(_lib.XR_ERR_RANGE, "state array legal: bits beyond the nets of the region a slot plays")
        pop = np.unpackbits(words.view(np.uint8), axis=1).sum(axis=1)
        if not np.array_equal(pop, staged["nlegal"].cpu().numpy().reshape(-1).astype(np.int64)):
            raise _lib.XRouteError(_lib.XR_ERR_RANGE, "state array nlegal: not the number of legal bits")

    def _store_arrays(self, arrays: dict):
        with torch.cuda.device(self.device):
            for k in self._STATE:              # (restore order matters: see _STATE)
                if k not in arrays:
                    continue
                sel = self._FETCH[k][0]
                t = arrays[k]
                _lib.check(self.L.xr_batch_store(self._h, sel, C.c_void_p(t.data_ptr()), t.numel() * t.element_size(),
                                                 _stream_ptr(self.device)))
            torch.cuda.current_stream(self.device).synchronize()          # the staging tensors die with the caller's frame

    def legal_sets(self) -> List[set]:
        """netSet of every env as Python sets of 1-based ids (host sync)."""
        words = self.fetch("legal").cpu().numpy().view(np.uint64)
        out = []
        for e in range(self.n_envs):
            s = set()
            for w in range(self.legal_words):
                m = int(words[e, w])
                while m:
                    b = (m & -m).bit_length() - 1
                    s.add(w * 64 + b + 1)
                    m &= m - 1
            out.append(s)
        return out

    def records(self) -> np.ndarray:
        """The packed per-env result records (xr_step_record) as a host structured array: ONE device->host copy."""
        raw = self.fetch("record").cpu().numpy()
        return raw.view(RECORD_DTYPE).reshape(self.n_envs)

    def total_steps(self) -> int:
        return int(self.fetch("steps").item())
