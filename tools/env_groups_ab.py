#!/usr/bin/env python3
"""A/B of env groups (xr_batch_set_groups / xr_batch_step_group): lock-step xr_batch_step* against S = 1, 2, 4, 8 groups, each group on
its own stream, every group stepping once per env-step (the same work as one lock-step step), variants alternated in one process.

Points: c5_1024    BASELINE config 5 regions (256x256x12, K = 32), 1024 slots, route only
        i512 / i1024   ispd18_test1-sized regions (24x40x9, K ~ U[4,36], config 4), full step in place
        i4096      the same, 4096 slots in place

One JSON line per (point, variant): ms per env-step (a step of every slot), env-steps/s, and whether every slot's hash chain equals a
lock-step twin's at the same env_steps.  Without --point the tool runs every point in a child process under its own `timeout` and stops
at the first one that fails.

    python tools/env_groups_ab.py [--steps 20] [--warmup 5] [--reps 3] [--point c5_1024]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POINTS = {"c5_1024": (5, 1024, "route", 32), "i512": (4, 512, "inplace", 256), "i1024": (4, 1024, "inplace", 256),
          "i4096": (4, 4096, "inplace", 256)}
VARIANTS = ("lockstep", 1, 2, 4, 8)
SEED = 77


def run_point(name, steps, warmup, reps):
    import numpy as np
    import torch
    from xroute_env_amd.batch import RegionBatch, partition_bounds
    from xroute_env_amd.regions import config_regions
    config, n, mode, n_regions = POINTS[name]
    regions = config_regions(config, n_regions)
    dev = "cuda:0"
    lock = RegionBatch(regions, n_envs=n, device=dev, auto_reset=True)
    grp = RegionBatch(regions, n_envs=n, device=dev, auto_reset=True)
    obs = {}
    for b in (lock, grp):
        b.reset(rotate=True)
        if mode == "inplace":
            obs[id(b)] = b.alloc_observation().zero_()
            b.observation(obs[id(b)])
    cur = torch.cuda.current_stream()
    streams = [torch.cuda.Stream() for _ in range(8)]
    act = torch.empty(n, dtype=torch.int32, device=dev)
    done_steps = {id(lock): 0, id(grp): 0}

    def lock_steps(k):
        for _ in range(k):
            lock.random_actions(SEED, act)
            if mode == "route":
                lock.step(act)
            else:
                lock.step(act, obs[id(lock)], inplace=True)
        done_steps[id(lock)] += k

    def group_steps(k):
        o = obs.get(id(grp))
        G = grp.n_groups
        for s in streams[:G]:
            s.wait_stream(cur)
        for _ in range(k):
            for g in range(G):
                lo, hi = grp.group_bounds(g)
                s = streams[g]
                with torch.cuda.stream(s):
                    grp.random_actions_group(g, SEED, out=act_g[g], stream=s)
                    if mode == "route":
                        grp.step_group(g, act_g[g], stream=s)
                    else:
                        grp.step_group(g, act_g[g], o[lo:hi], inplace=True, stream=s)
        for s in streams[:G]:
            cur.wait_stream(s)
        done_steps[id(grp)] += k

    times = {v: [] for v in VARIANTS}
    act_g = []
    for rep in range(reps):
        for v in VARIANTS:
            if v != "lockstep":
                torch.cuda.synchronize()
                grp.set_groups(partition_bounds(v, n))
                act_g = []
                for g in range(v):
                    lo, hi = grp.group_bounds(g)
                    with torch.cuda.stream(streams[g]):
                        act_g.append(torch.empty(hi - lo, dtype=torch.int32, device=dev))
                torch.cuda.synchronize()
            fn = lock_steps if v == "lockstep" else group_steps
            fn(warmup)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(steps)
            e1.record()
            e1.synchronize()
            times[v].append(e0.elapsed_time(e1) / steps)
    # hash chains: bring the lock-step twin to the grouped batch's step count, compare every slot
    torch.cuda.synchronize()
    lock_steps(done_steps[id(grp)] - done_steps[id(lock)])
    torch.cuda.synchronize()
    match = bool(torch.equal(lock.fetch("hash"), grp.fetch("hash")) and torch.equal(lock.fetch("env_steps"), grp.fetch("env_steps")))
    for v in VARIANTS:
        ms = float(np.median(times[v]))
        print(json.dumps({"point": name, "envs": n, "mode": mode, "variant": "lockstep" if v == "lockstep" else f"groups{v}",
                          "ms_per_step": round(ms, 4), "env_steps_per_s": round(n / ms * 1e3), "reps_ms": [round(t, 4) for t in times[v]],
                          "hash_match": match}), flush=True)
    return match


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--point", choices=list(POINTS))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per point (child processes)")
    a = ap.parse_args()
    if a.point:
        sys.exit(0 if run_point(a.point, a.steps, a.warmup, a.reps) else 1)
    for p in POINTS:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--point", p, "--steps", str(a.steps),
               "--warmup", str(a.warmup), "--reps", str(a.reps)]
        rc = subprocess.call(cmd)
        if rc != 0:
            print(json.dumps({"point": p, "error": f"exit status {rc}"}), flush=True)
            sys.exit(rc)


if __name__ == "__main__":
    main()
