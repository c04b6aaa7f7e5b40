#!/usr/bin/env python3
"""What the weighted pick costs inside a rollout (xr_batch_rollout_weighted), on the 4096-slot ispd18_test1 pack at the stationary
nets-left distribution, 16 rollouts per env, HIP events, 7 repetitions:

  (a) XR_ROLLOUT_RANDOM through xr_batch_rollout;
  (b) XR_ROLLOUT_WEIGHTED with unit weights through xr_batch_rollout_weighted — first asserted to give (a)'s outputs bit for bit;
      the timed runs of (a) and (b) alternate;
  (c) (a) on a checkout of the PARENT commit (--parent-root: a tree with its own built library), in a process of its own, in the same
      session.

No ratio is fixed in advance.  The yardstick for (a) is (c): (a)'s median must lie inside (c)'s min-max range widened by that range's
own width; the yardstick for (b) is (a), with the same margin — the run-to-run spread this very run shows.  Beside them, for the record
only: `weighted_actions` and `random_actions` at the same 4096 envs.  One child process per tree under a `timeout`; nothing is started
after a failure.

    python tools/weighted_ab.py [--parent-root DIR] [--envs 4096] [--rollouts 16] [--json profiles/weighted_ab.json]
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 417


def timed_once(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def run(root, n, R, settle, reps, weighted):
    """The child: the package of `root` (this tree, or the parent's).  weighted = False: (a) alone, which every tree can run."""
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from xroute_env_amd.batch import RegionBatch
    from xroute_env_amd.lefdef import load_region_pack
    regions = load_region_pack(os.path.join(HERE, "tests", "golden", "ispd18_test1_regions.npz"))
    dev = "cuda:0"
    b = RegionBatch(regions, n_envs=n, device=dev, auto_reset=True)
    b.reset()
    act = torch.empty(n, dtype=torch.int32, device=dev)
    for s in range(settle):                    # to the stationary nets-left distribution
        b.step(b.random_actions(SEED + s, act))
    nl = b.fetch("nlegal").cpu().numpy()
    routes = int(nl.sum()) * R
    ra = b.rollout(R, SEED)
    bufs = lambda r: dict(out=r["out"], return_out=r["ret"], hash_out=r["hash"], order_out=r["order"])
    roll_a = lambda: b.rollout(R, SEED, **bufs(ra))
    rec = {"envs": n, "rollouts": R, "k_max": b.k_max, "rollout_routes": routes, "mean_nets_left": round(float(nl.mean()), 3)}
    if not weighted:
        for _ in range(2):
            roll_a()
        rec["random_ms"] = [round(timed_once(roll_a), 3) for _ in range(reps)]
        print(json.dumps(rec), flush=True)
        return True
    w = torch.ones((n, b.k_max), dtype=torch.int32, device=dev)
    rb = b.rollout(R, SEED, policy="weighted", weights=w)
    torch.cuda.synchronize()
    same = all(torch.equal(ra[k], rb[k]) for k in ("out", "hash", "order")) and torch.equal(ra["ret"].view(torch.int64), rb["ret"].view(torch.int64))
    assert same, "XR_ROLLOUT_WEIGHTED with unit weights differs from XR_ROLLOUT_RANDOM"
    roll_b = lambda: b.rollout(R, SEED, policy="weighted", weights=w, **bufs(rb))
    for _ in range(2):
        roll_a(); roll_b()
    ta, tb = [], []
    for i in range(reps):                      # alternated, and who goes first alternates too
        for which in ((0, 1) if i % 2 == 0 else (1, 0)):
            (tb if which else ta).append(timed_once(roll_b if which else roll_a))
    # the picks alone, for the record: 100 calls each
    out = torch.empty(n, dtype=torch.int32, device=dev)
    pick_r = lambda: [b.random_actions(SEED + i, out) for i in range(100)]
    pick_w = lambda: [b.weighted_actions(w, SEED + i, out) for i in range(100)]
    pick_r(); pick_w()
    tr, tw = [], []
    for i in range(reps):
        tr.append(timed_once(pick_r) / 100)
        tw.append(timed_once(pick_w) / 100)
    rec.update(same_outputs=bool(same), random_ms=[round(t, 3) for t in ta], weighted_ms=[round(t, 3) for t in tb],
               random_actions_us=[round(t * 1e3, 2) for t in tr], weighted_actions_us=[round(t * 1e3, 2) for t in tw])
    print(json.dumps(rec), flush=True)
    return same


def inside(x, ref):
    """x inside ref's min-max range widened by that range's own width."""
    lo, hi = min(ref), max(ref)
    return lo - (hi - lo) <= x <= hi + (hi - lo)


def child(root, a, weighted):
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--envs", str(a.envs),
           "--rollouts", str(a.rollouts), "--settle", str(a.settle), "--reps", str(a.reps)] + (["--weighted"] if weighted else [])
    r = subprocess.run(cmd, capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    lines = [json.loads(s) for s in r.stdout.splitlines() if s.startswith("{")]
    if r.returncode != 0 or not lines:
        print(json.dumps({"error": f"exit status {r.returncode}", "stderr": r.stderr[-2000:]}), flush=True)
        sys.exit(1)
    return lines[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rollouts", type=int, default=16)
    ap.add_argument("--settle", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=280)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built: measures (c)")
    ap.add_argument("--json", default=os.path.join(HERE, "profiles", "weighted_ab.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--weighted", action="store_true")
    a = ap.parse_args()
    if a.child:
        sys.exit(0 if run(a.root, a.envs, a.rollouts, a.settle, a.reps, a.weighted) else 1)
    med = lambda v: sorted(v)[len(v) // 2]
    parent = child(os.path.abspath(a.parent_root), a, False) if a.parent_root else None
    here = child(HERE, a, True)
    rec = {"tool": "tools/weighted_ab.py", **{k: here[k] for k in ("envs", "rollouts", "k_max", "rollout_routes", "mean_nets_left", "same_outputs")},
           "a_random_ms": here["random_ms"], "b_weighted_unit_ms": here["weighted_ms"],
           "a_median_ms": med(here["random_ms"]), "b_median_ms": med(here["weighted_ms"]),
           "b_over_a": round(med(here["weighted_ms"]) / med(here["random_ms"]), 4),
           "b_inside_a_range_widened_by_its_width": inside(med(here["weighted_ms"]), here["random_ms"]),
           "random_actions_us": here["random_actions_us"], "weighted_actions_us": here["weighted_actions_us"],
           "random_actions_median_us": med(here["random_actions_us"]), "weighted_actions_median_us": med(here["weighted_actions_us"])}
    if parent:
        assert parent["rollout_routes"] == here["rollout_routes"], "the parent's batch is in another state"
        rec.update(c_parent_random_ms=parent["random_ms"], c_median_ms=med(parent["random_ms"]),
                   a_over_c=round(med(here["random_ms"]) / med(parent["random_ms"]), 4),
                   a_inside_c_range_widened_by_its_width=inside(med(here["random_ms"]), parent["random_ms"]))
    else:
        rec.update(c_parent_random_ms=None, note="(c) not measured: no --parent-root")
    print(json.dumps(rec), flush=True)
    with open(a.json, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
