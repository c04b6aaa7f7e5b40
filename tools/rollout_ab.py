#!/usr/bin/env python3
"""What rollouts cost (xr_batch_rollout), on the 4096-slot ispd18_test1 pack at the stationary nets-left distribution:

  (i)   one `rollout` with R = 8: every env's episode played to its end 8 times, one persistent launch;
  (ii)  the same table without it — the only way the API offered before: `state_dict`, step to done with
        `random_actions(rollout_seed(seed, r))`, read the totals, `load_state_dict`; R rounds.  Checked to yield the same table first;
  (iii) the route-only `step` rate (random net-order policy), for scale.

Records rollout-routes/s of (i), the ratio (ii)/(i), and rollout-routes/s over route-only env-steps/s.  HIP events around each timed block,
warm-up before it, median of the repetitions.  One child process under a `timeout`; nothing is started after a failure.

    python tools/rollout_ab.py [--envs 4096] [--rollouts 8] [--json profiles/rollout_ab.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 417


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


def run(n, R, settle, reps):
    import numpy as np
    import torch
    from xroute_env_amd import _lib
    from xroute_env_amd.batch import RegionBatch
    from xroute_env_amd.lefdef import load_region_pack
    regions = load_region_pack(os.path.join(ROOT, "tests", "golden", "ispd18_test1_regions.npz"))
    dev = "cuda:0"
    b = RegionBatch(regions, n_envs=n, device=dev, auto_reset=True)
    b.reset()
    act = torch.empty(n, dtype=torch.int32, device=dev)
    for s in range(settle):                    # to the stationary nets-left distribution
        b.step(b.random_actions(SEED + s, act))
    k = b.k_max
    nl = b.fetch("nlegal").cpu().numpy()
    routes = int(nl.sum()) * R                 # every rollout routes every net its env has left

    # (i)
    res = b.rollout(R, SEED)
    roll = lambda: b.rollout(R, SEED, out=res["out"], return_out=res["ret"], hash_out=res["hash"], order_out=res["order"])
    for _ in range(2):
        roll()
    t_roll = timed(roll, reps + 2)
    ms_roll = float(np.median(t_roll))
    table = {key: v.cpu().numpy().copy() for key, v in res.items()}
    assert int(table["out"][:, :, 4].sum()) == routes

    # (ii) snapshot, step to done under the rollout's seed, restore.  The batch restarts finished envs (auto_reset), so an env is followed
    # only while it has nets left and its first done ends it.
    got_delta, got_ret = np.zeros((n, R, 3), np.int64), np.zeros((n, R), np.float64)
    got_hash, got_order = np.zeros((n, R), np.int64), np.zeros((n, R, k), np.int32)
    most = int(nl.max())

    def by_steps(collect):
        sd = b.state_dict()
        for r in range(R):
            seed_r = _lib.rollout_seed(SEED, r)
            live = nl > 0
            if collect:
                got_hash[:, r] = b.fetch("hash").cpu().numpy()
            for ply in range(most):
                b.random_actions(seed_r, act)
                if collect:
                    a = act.cpu().numpy()
                b.step(act)
                if collect:
                    rec = b.records()
                    h = b.fetch("hash").cpu().numpy()
                    idx = np.flatnonzero(live)
                    got_delta[idx, r] += rec["delta"][idx]
                    got_ret[idx, r] = got_ret[idx, r] + rec["reward"][idx]
                    got_order[idx, r, ply] = a[idx]
                    got_hash[idx, r] = h[idx]
                    live = live & (rec["done"] == 0)
                else:
                    b.fetch("record")
            b.load_state_dict(sd)

    by_steps(True)
    same = bool(np.array_equal(got_delta, table["out"][:, :, :3]) and np.array_equal(got_ret.view(np.uint64), table["ret"].view(np.uint64))
                and np.array_equal(got_hash, table["hash"]) and np.array_equal(got_order, table["order"]))
    t_steps = timed(lambda: by_steps(False), max(1, reps - 1))
    ms_steps = float(np.median(t_steps))

    # (iii) route-only step rate
    def steps20():
        for s in range(20):
            b.step(b.random_actions(SEED + 1000 + s, act))
    steps20()
    t_route = timed(steps20, reps)
    ms_route = float(np.median(t_route)) / 20
    per_cu, lds = b.route_occupancy()
    rec = {"tool": "tools/rollout_ab.py", "envs": n, "rollouts": R, "k_max": k, "rollout_routes": routes, "mean_nets_left": round(float(nl.mean()), 3),
           "max_nets_left": most, "rollout_ms": round(ms_roll, 3), "rollout_routes_per_s": round(routes / ms_roll * 1e3),
           "snapshot_step_restore_ms": round(ms_steps, 2), "same_table": same, "speedup": round(ms_steps / ms_roll, 1),
           "route_only_step_ms": round(ms_route, 4), "route_only_env_steps_per_s": round(n / ms_route * 1e3),
           "rollout_routes_per_env_step_rate": round((routes / ms_roll) / (n / ms_route), 3), "route_workgroups_per_cu": per_cu,
           "reps_ms": {"rollout": [round(t, 3) for t in t_roll], "snapshot_step_restore": [round(t, 1) for t in t_steps],
                       "route_only_x20": [round(t, 3) for t in t_route]}}
    print(json.dumps(rec), flush=True)
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rollouts", type=int, default=8)
    ap.add_argument("--settle", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "rollout_ab.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        sys.exit(0 if run(a.envs, a.rollouts, a.settle, a.reps) else 1)
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--envs", str(a.envs), "--rollouts", str(a.rollouts),
           "--settle", str(a.settle), "--reps", str(a.reps)]
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
