#!/usr/bin/env python3
"""What a branch costs (xr_batch_branch), on the 4096-slot ispd18_test1 pack at the stationary nets-left distribution, under a seeded
map in which every slot moves (so every parent is itself overwritten: the two-pass worst case, every row staged):

  (i)   `branch`;
  (i')  `branch` under a map in which half the slots take the state of a slot that stays (one pass, nothing staged), for scale;
  (ii)  the device route the API offered before: `fetch` -> `index_select` -> `xr_batch_store` per state array (three of the stores
        validate on the host and synchronise);
  (iii) `state_dict` -> index -> `load_state_dict`;
  (iv)  a plain device-to-device copy of the bytes a branch of every slot moves once (the bandwidth yardstick).

First asserts that (i), (ii) and (iii) produce the same state.  Then beam search (envs/beam.py) of width 4 and 8 over the pack: the time
of a ply beside one lookahead and one route-only step of the same batch, and the mean episode cost.  HIP events around each timed block,
warm-up before it, medians of the repetitions.  One child process under a `timeout`; nothing is started after a failure.

    python tools/branch_ab.py [--envs 4096] [--json profiles/branch_ab.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 431


def timed(fn, reps):
    import torch
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def run(n, settle, reps, beam_regions):
    import ctypes as C
    import numpy as np
    import torch
    from xroute_env_amd import _lib
    from xroute_env_amd.batch import RegionBatch
    from xroute_env_amd.envs.beam import beam_search
    from xroute_env_amd.lefdef import load_region_pack
    regions = load_region_pack(os.path.join(ROOT, "tests", "golden", "ispd18_test1_regions.npz"))
    dev = "cuda:0"
    b = RegionBatch(regions, n_envs=n, device=dev, auto_reset=True)
    b.reset()
    act = torch.empty(n, dtype=torch.int32, device=dev)
    for s in range(settle):                    # to the stationary nets-left distribution
        b.step(b.random_actions(SEED + s, act))
    rng = np.random.default_rng(SEED)
    i = np.arange(n)
    every = (i + 1 + rng.integers(0, n - 1, n)) % n                      # every slot moves; not injective
    assert (every != i).all() and len(set(every.tolist())) < n
    half = np.where(i % 2 == 0, -1, (2 * rng.integers(0, n // 2, n)) % n)      # odd slots take an even slot's state; even slots stay
    parent = torch.as_tensor(every.astype(np.int32), device=dev)
    parent_half = torch.as_tensor(half.astype(np.int32), device=dev)
    idx_dev = torch.as_tensor(every, device=dev)
    idx_cpu = torch.as_tensor(every)
    arrays = [k for k in b._STATE if k != "steps"]

    def by_store():
        got = {k: b.fetch(k).index_select(0, idx_dev).contiguous() for k in arrays}
        for k in arrays:              # (restore order: region first)
            t = got[k]
            _lib.check(b.L.xr_batch_store(b._h, b._FETCH[k][0], C.c_void_p(t.data_ptr()), t.numel() * t.element_size(), b._stream_arg(None)))
        return got

    def by_state_dict():
        sd = b.state_dict()
        b.load_state_dict({k: (v if k.startswith("_") or k == "steps" else v[idx_cpu].contiguous()) for k, v in sd.items()})

    def state():
        return {k: b.fetch(k).cpu().numpy().tobytes() for k in arrays}

    # the three routes give the same state
    sd0 = b.state_dict()
    b.branch(parent)
    s_branch = state()
    b.load_state_dict(sd0)
    by_store()
    torch.cuda.synchronize()
    s_store = state()
    b.load_state_dict(sd0)
    by_state_dict()
    s_dict = state()
    same = s_branch == s_store == s_dict
    assert same, "the three routes disagree"

    row_bytes = 2 * b.n_max + 4 * b.path_cap + 8 * b.legal_words + 125
    state_bytes = sum(len(v) for v in s_branch.values())               # what (ii) and (iii) carry: no path / sweeps / touched rows
    src = torch.empty(n * row_bytes, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    for _ in range(3):
        b.branch(parent); b.branch(parent_half); dst.copy_(src)
    x20 = lambda fn: [t / 20 for t in timed(lambda: [fn() for _ in range(20)], reps + 4)]      # (a call is ~0.1 ms: 20 per timed block)
    t_branch = x20(lambda: b.branch(parent))
    t_half = x20(lambda: b.branch(parent_half))
    t_copy = x20(lambda: dst.copy_(src))
    by_store()
    t_store = timed(by_store, reps)
    t_dict = timed(by_state_dict, max(2, reps - 1))
    med = lambda t: float(np.median(t))
    ms_branch, ms_half, ms_copy, ms_store, ms_dict = med(t_branch), med(t_half), med(t_copy), med(t_store), med(t_dict)
    nl = b.fetch("nlegal").cpu().numpy()
    rec = {"tool": "tools/branch_ab.py", "envs": n, "n_max": b.n_max, "path_cap": b.path_cap, "legal_words": b.legal_words,
           "row_bytes": row_bytes, "mean_nets_left": round(float(nl.mean()), 3), "same_state": same,
           "branch_every_slot_moves_ms": round(ms_branch, 4), "branch_bytes_read_and_written": 4 * n * row_bytes,
           "branch_half_from_keepers_ms": round(ms_half, 4), "branch_half_bytes_read_and_written": 2 * (n // 2) * row_bytes,
           "fetch_index_store_ms": round(ms_store, 3), "fetch_index_store_state_bytes": state_bytes,
           "state_dict_load_state_dict_ms": round(ms_dict, 2),
           "device_copy_ms": round(ms_copy, 4), "device_copy_bytes": n * row_bytes,
           "branch_over_device_copy": round(ms_branch / ms_copy, 2), "fetch_index_store_over_branch": round(ms_store / ms_branch, 1),
           "state_dict_over_branch": round(ms_dict / ms_branch, 1),
           "branch_GBps_read_plus_write": round(4 * n * row_bytes / ms_branch / 1e6, 1),
           "device_copy_GBps_read_plus_write": round(2 * n * row_bytes / ms_copy / 1e6, 1),
           "reps_ms": {"branch": [round(t, 4) for t in t_branch], "branch_half": [round(t, 4) for t in t_half],
                       "device_copy": [round(t, 4) for t in t_copy], "fetch_index_store": [round(t, 2) for t in t_store],
                       "state_dict": [round(t, 1) for t in t_dict]}}
    b.close()

    # beam search over the pack: a ply beside one lookahead and one route-only step of a batch of the same size
    beam = {}
    regs = regions[:beam_regions]
    for W in (1, 4, 8):
        stats = {}
        res = beam_search(regs, W, device=dev, stats=stats)
        cost = -float(np.mean([beams[0]["ret"] for beams in res]))
        q = RegionBatch(regs, n_envs=len(regs) * W, device=dev, auto_reset=True)
        q.assign([r for r in range(len(regs)) for _ in range(W)])
        q.reset()
        a = torch.empty(q.n_envs, dtype=torch.int32, device=dev)
        for s in range(3):
            q.step(q.random_actions(SEED + s, a))
        out, rew = q.lookahead()
        t_look = timed(lambda: q.lookahead(out=out, reward_out=rew), reps + 2)
        t_step = timed(lambda: q.step(q.random_actions(SEED + 9, a)), reps + 2)
        q.close()
        beam[f"W{W}"] = {"slots": len(regs) * W, "plies": len(stats["ply_ms"]), "mean_best_episode_cost": round(cost, 2),
                         "ply_ms_median": round(med(stats["ply_ms"][1:]), 3), "ply_ms_first": round(stats["ply_ms"][0], 3),
                         "lookahead_ms": round(med(t_look), 3), "route_only_step_ms": round(med(t_step), 4)}
    rec["beam"] = {"regions": len(regs), **beam}
    print(json.dumps(rec), flush=True)
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--settle", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--beam-regions", type=int, default=256)
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "branch_ab.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        sys.exit(0 if run(a.envs, a.settle, a.reps, a.beam_regions) else 1)
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--envs", str(a.envs),
           "--settle", str(a.settle), "--reps", str(a.reps), "--beam-regions", str(a.beam_regions)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    lines = [json.loads(s) for s in r.stdout.splitlines() if s.startswith("{")]
    if r.returncode != 0 or not lines:
        print(json.dumps({"error": f"exit status {r.returncode}", "stderr": r.stderr[-2000:]}), flush=True)
        sys.exit(1)
    with open(a.json, "w") as fh:
        json.dump(lines[-1], fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
