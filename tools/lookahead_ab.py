#!/usr/bin/env python3
"""What a lookahead costs (xr_batch_lookahead), on the 4096-slot ispd18_test1 pack at the stationary nets-left distribution:

  (i)   one `lookahead` of every candidate of every env;
  (ii)  the same table without it — the only way the API offered before: `state_dict`, then per candidate rank one route-only `step`
        (every env picks its rank-th legal net), read the deltas, `load_state_dict`; k_max rounds.  Checked to yield the same table first;
  (iii) the route-only `step` rate (random net-order policy).

Records candidate-routes/s of (i), the ratio (ii)/(i) per decision, and candidate-routes/s over route-only env-steps/s.  HIP events around
each timed block, warm-up before it, median of the repetitions.  One child process under a `timeout`; nothing is started after a failure.

    python tools/lookahead_ab.py [--envs 4096] [--json profiles/lookahead_ab.json]
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


def run(n, settle, reps):
    import numpy as np
    import torch
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
    cands = int(nl.sum())

    # (i)
    ds, rw = b.lookahead()
    look = lambda: b.lookahead(out=ds, reward_out=rw)
    for _ in range(3):
        look()
    t_look = timed(lambda: [look() for _ in range(10)], reps)
    ms_look = float(np.median(t_look)) / 10
    table, table_rw = ds.cpu().numpy().copy(), rw.cpu().numpy().copy()

    # (ii) snapshot, one route-only step per candidate rank, restore
    words = b.fetch("legal").cpu().numpy().view(np.uint64)
    bits = ((words[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).astype(bool).reshape(n, -1)
    rank_net = np.zeros((n, k), np.int32)      # rank_net[e, r] = the r-th legal net of env e (0: it has fewer)
    for e in range(n):
        ids = np.flatnonzero(bits[e]) + 1
        rank_net[e, :ids.size] = ids
    rank_act = torch.from_numpy(rank_net.T.copy()).to(dev)
    got = np.zeros_like(table); got[:, :, 3] = -1
    got_rw = np.full_like(table_rw, -np.inf)

    def by_steps(collect):
        sd = b.state_dict()
        for r in range(k):
            b.step(rank_act[r])
            if collect:
                rec = b.records()
                live = np.flatnonzero(rank_net[:, r] > 0)
                got[live, rank_net[live, r] - 1, :3] = rec["delta"][live]
                got[live, rank_net[live, r] - 1, 3] = rec["status"][live]
                got_rw[live, rank_net[live, r] - 1] = rec["reward"][live]
            else:
                b.fetch("record")
            b.load_state_dict(sd)

    by_steps(True)
    same = bool(np.array_equal(got, table) and np.array_equal(got_rw.view(np.uint64), table_rw.view(np.uint64)))
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
    rec = {"tool": "tools/lookahead_ab.py", "envs": n, "k_max": k, "candidates": cands, "mean_nets_left": round(float(nl.mean()), 3),
           "lookahead_ms": round(ms_look, 4), "candidate_routes_per_s": round(cands / ms_look * 1e3),
           "snapshot_step_restore_ms": round(ms_steps, 2), "same_table": same,
           "speedup_per_decision": round(ms_steps / ms_look, 1),
           "route_only_step_ms": round(ms_route, 4), "route_only_env_steps_per_s": round(n / ms_route * 1e3),
           "candidate_routes_per_env_step_rate": round((cands / ms_look) / (n / ms_route), 3),
           "route_workgroups_per_cu": per_cu,
           "reps_ms": {"lookahead_x10": [round(t, 3) for t in t_look], "snapshot_step_restore": [round(t, 1) for t in t_steps],
                       "route_only_x20": [round(t, 3) for t in t_route]}}
    print(json.dumps(rec), flush=True)
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--settle", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "lookahead_ab.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        sys.exit(0 if run(a.envs, a.settle, a.reps) else 1)
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--envs", str(a.envs), "--settle", str(a.settle),
           "--reps", str(a.reps)]
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
