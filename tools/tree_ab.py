#!/usr/bin/env python3
"""What the tree search costs as one call (xr_batch_tree_search) against the same search driven from the host, on the 4096-slot
ispd18_test1 pack at the stationary nets-left distribution, 8 waves x 8 lanes:

  (i)   `RegionBatch.tree_search`: reset, then select / rollout / backup per wave, all enqueued, one synchronise at the end;
  (ii)  the host form a user had before: XR-Tree v1 in Python (tests/tree_twin.py: select and backup per row on the host) around one
        `RegionBatch.rollout` per wave — a prefix upload and a read of the returns and orders per wave;
  (iii) the eight rollout launches of (i) alone, with the very prefixes (i) selected: what is left of (i) is select + backup + reset.

First asserts that (i) and (ii) give the same paths, returns, visit counts, values and best lines, bit for bit.  HIP events around
(i) and (iii), a host clock around (ii) (it ends in device reads); warm-up before each, (i) and (iii) alternated, medians of the
repetitions.  One child process under a `timeout`; nothing is started after a failure.

    python tools/tree_ab.py [--envs 4096] [--json profiles/tree_ab.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 977


def run(n, settle, reps, host_reps, n_waves, n_par):
    import numpy as np
    import torch
    from tests import tree_twin
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
    K, S = max(b.k_max, 1), n_waves * n_par
    cap = 1 + (S + 1) * K
    words = b.fetch("legal").cpu().numpy().view(np.uint64)
    bits = ((words[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).astype(bool).reshape(n, -1)[:, :K]
    legal = [(np.flatnonzero(row) + 1).tolist() for row in bits]
    E = _lib.tree_exploration_table(1.25, 19652.0, S)

    def device_form():
        return b.tree_search(n_waves, n_par, SEED, node_cap=cap, trace=True)

    def host_form():
        def evaluate(w, paths):
            prefix = np.zeros((n, n_par, K), np.int32)
            for r in range(n):
                for j in range(n_par):
                    prefix[r, j, :len(paths[r][j])] = paths[r][j]
            res = b.rollout(n_par, _lib.tree_seed(SEED, w), prefix=torch.from_numpy(prefix).to(dev))
            return res["ret"].cpu().numpy().tolist(), res["order"].cpu().numpy().tolist()
        return tree_twin.search(legal, n_waves, n_par, cap, E, evaluate, K)

    # the two forms give the same search
    d = {k: v.cpu().numpy() for k, v in device_form().items()}
    t0 = time.perf_counter()
    results, paths, returns, _ = host_form()
    host_s = [time.perf_counter() - t0]
    same = (np.array_equal(np.array(paths, np.int32).reshape(n, S, K), d["paths"])
            and np.array_equal(np.array(returns, np.float64).view(np.uint64).reshape(n, S), d["returns"].view(np.uint64))
            and np.array_equal(np.array([r["visits"] for r in results], np.int32), d["visits"])
            and np.array_equal(np.array([r["value"] for r in results], np.float64).view(np.uint64), d["value"].view(np.uint64))
            and np.array_equal(np.array([r["info"] for r in results], np.int32), d["info"])
            and np.array_equal(np.array([r["best_order"] for r in results], np.int32), d["best_order"])
            and np.array_equal(np.array([r["best_return"] for r in results], np.float64).view(np.uint64), d["best_return"].view(np.uint64)))
    assert same, "the device search and the host-driven search disagree"
    for _ in range(host_reps - 1):
        t0 = time.perf_counter()
        host_form()
        host_s.append(time.perf_counter() - t0)

    prefixes = [torch.from_numpy(np.ascontiguousarray(d["paths"][:, w * n_par:(w + 1) * n_par])).to(dev) for w in range(n_waves)]
    bufs = b.rollout(n_par, SEED)
    kw = dict(out=bufs["out"], return_out=bufs["ret"], hash_out=bufs["hash"], order_out=bufs["order"])

    def rollouts_alone():
        for w in range(n_waves):
            b.rollout(n_par, _lib.tree_seed(SEED, w), prefix=prefixes[w], **kw)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(2):
        device_form(); rollouts_alone()
    torch.cuda.synchronize()
    t_tree, t_roll = [], []
    for _ in range(reps):                      # alternated
        t_tree.append(timed(device_form))
        t_roll.append(timed(rollouts_alone))
    med = lambda t: float(np.median(t))
    ms_tree, ms_roll, ms_host = med(t_tree), med(t_roll), med(host_s) * 1e3
    nl = b.fetch("nlegal").cpu().numpy()
    routed = S * int(nl.sum())                 # every simulation routes all the nets its env has left
    rec = {"tool": "tools/tree_ab.py", "envs": n, "n_waves": n_waves, "n_par": n_par, "simulations_per_env": S, "k_max": K, "node_cap": cap,
           "mean_nets_left": round(float(nl.mean()), 3), "live_envs": int((nl > 0).sum()), "routed_nets_per_search": routed, "same_search": same,
           "device_form_ms": round(ms_tree, 3), "host_form_ms": round(ms_host, 1), "rollout_launches_alone_ms": round(ms_roll, 3),
           "host_over_device": round(ms_host / ms_tree, 1),
           "select_backup_reset_ms": round(ms_tree - ms_roll, 3), "select_backup_reset_share": round((ms_tree - ms_roll) / ms_tree, 4),
           "mean_nodes_used": round(float(d["info"][nl > 0, 1].mean()), 1), "mean_max_depth": round(float(d["info"][nl > 0, 2].mean()), 2),
           "pool_full_rows": int((d["info"][:, 3] != 0).sum()),
           "reps_ms": {"device_form": [round(t, 3) for t in t_tree], "rollout_launches_alone": [round(t, 3) for t in t_roll],
                       "host_form": [round(t * 1e3, 1) for t in host_s]}}
    b.close()
    print(json.dumps(rec), flush=True)
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--settle", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--waves", type=int, default=8)
    ap.add_argument("--par", type=int, default=8)
    ap.add_argument("--timeout", type=int, default=540)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "tree_ab.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        sys.exit(0 if run(a.envs, a.settle, a.reps, a.host_reps, a.waves, a.par) else 1)
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--envs", str(a.envs),
           "--settle", str(a.settle), "--reps", str(a.reps), "--host-reps", str(a.host_reps), "--waves", str(a.waves), "--par", str(a.par)]
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
