#!/usr/bin/env python3
"""What tree reuse costs and carries (xr_batch_tree_search_keep), on the 4096-slot ispd18_test1 pack at the stationary nets-left
distribution, 8 waves x 8 lanes, HIP events, warm-up first, 7 repetitions alternated:

  (a) `RegionBatch.tree_search` on a build of the PARENT commit (--parent DIR: a checkout of the parent with its library built; a process
      of its own, run before and after this commit's), against
  (b) the same call on this commit: it must lie inside (a)'s range widened by its own width;
  (c) the kept call with played = None (a fresh search that leaves its tree behind), alternated with (b), same yardstick against (b);
  (d) the kept call after one real step, with played = the actions stepped, alternated with (b) at the same states: its time, the
      share of live rows that kept a tree, the mean carried visits and nodes per live row.
The first kernel of (c) and (d) on its own comes from the kernel records of torch.profiler (null where it gives none).
Child processes under a `timeout`; nothing is started after a failure.

    python tools/tree_keep_ab.py [--parent DIR] [--envs 4096] [--json profiles/tree_keep_ab.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 977


def _setup(root, n, settle):
    sys.path.insert(0, root)
    import torch
    from xroute_env_amd.batch import RegionBatch
    from xroute_env_amd.lefdef import load_region_pack
    regions = load_region_pack(os.path.join(ROOT, "tests", "golden", "ispd18_test1_regions.npz"))
    b = RegionBatch(regions, n_envs=n, device="cuda:0", auto_reset=True)
    b.reset()
    act = torch.empty(n, dtype=torch.int32, device="cuda:0")
    for s in range(settle):                    # to the stationary nets-left distribution
        b.step(b.random_actions(SEED + s, act))
    return torch, b


def _timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def run_plain(root, n, settle, reps, n_waves, n_par):
    torch, b = _setup(root, n, settle)
    cap = 1 + (n_waves * n_par + 1) * max(b.k_max, 1)
    fn = lambda: b.tree_search(n_waves, n_par, SEED, node_cap=cap)
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t = [_timed(torch, fn)[0] for _ in range(reps)]
    res = fn()
    digest = int(res["visits"].to(torch.int64).sum()) * 1000003 + int(res["info"][:, 1].to(torch.int64).sum())
    print(json.dumps({"plain_ms": [round(x, 3) for x in t], "digest": digest, "library": os.path.join(root, "xroute_env_amd")}), flush=True)
    b.close()


def _begin_kernel_us(torch, fn):
    """The device time of xr_tree_keep_begin_kernel in one call of fn, from torch.profiler's kernel records (None: no such record)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        for ev in prof.events():
            if "xr_tree_keep_begin_kernel" in ev.name:
                us = getattr(ev, "device_time", None)
                return float(us if us is not None else ev.cuda_time)
    except Exception as exc:          # the measurement is optional: say why it is missing
        print(json.dumps({"profiler": repr(exc)[:300]}), flush=True)
    return None


def run_keep(root, n, settle, reps, n_waves, n_par):
    import numpy as np
    torch, b = _setup(root, n, settle)
    from xroute_env_amd import _lib
    from xroute_env_amd.envs.vector_env import XRouteVectorEnv
    K, S = max(b.k_max, 1), n_waves * n_par
    cap = 1 + 2 * (S + 1) * K
    plain = lambda: b.tree_search(n_waves, n_par, SEED, node_cap=cap)
    fresh = lambda: b.tree_search(n_waves, n_par, SEED, node_cap=cap, keep=True)
    for _ in range(2):
        plain(); fresh()
    torch.cuda.synchronize()
    same = all(torch.equal(x, y) for x, y in zip((plain()[k] for k in ("visits", "info", "best_order")), (fresh()[k] for k in ("visits", "info", "best_order"))))
    t_b, t_c = [], []
    for _ in range(reps):                      # alternated
        t_b.append(_timed(torch, plain)[0])
        t_c.append(_timed(torch, fresh)[0])
    begin_c = _begin_kernel_us(torch, fresh)
    # (d): search, step the most visited net, continue — every repetition is the search after one real step
    res = fresh()
    t_b2, t_d, kept_share, visits, nodes, begin_d, full = [], [], [], [], [], None, 0
    for r in range(reps + 2):
        act = XRouteVectorEnv._most_visited(res)
        b.step(act)
        nl = b.fetch("nlegal")
        if r == 0:                             # (one unmeasured round: the continued call's first)
            res = b.tree_search(n_waves, n_par, SEED + r, node_cap=cap, keep=True, played=act)
            continue
        if r == reps + 1:                      # (and one under the profiler, for the first kernel alone)
            begin_d = _begin_kernel_us(torch, lambda: b.tree_search(n_waves, n_par, SEED + r, node_cap=cap, keep=True, played=act))
            break
        t_b2.append(_timed(torch, lambda: b.tree_search(n_waves, n_par, SEED + r, node_cap=cap))[0])
        ms, res = _timed(torch, lambda: b.tree_search(n_waves, n_par, SEED + r, node_cap=cap, keep=True, played=act))
        t_d.append(ms)
        live = nl > 0
        kept = res["kept"][live].to(torch.float64)
        kept_share.append(float(((res["info"][live, 3] & _lib.XR_TREE_KEPT) != 0).to(torch.float64).mean()))
        visits.append(float(kept[:, 0].mean())); nodes.append(float(kept[:, 1].mean()))
        full += int(((res["info"][:, 3] & _lib.XR_TREE_POOL_FULL) != 0).sum())
    med = lambda t: round(float(np.median(t)), 3)
    print(json.dumps({"n_waves": n_waves, "n_par": n_par, "node_cap": cap, "k_max": K, "fresh_kept_call_equals_plain": bool(same),
                      "b_plain_ms": med(t_b), "c_keep_fresh_ms": med(t_c), "c_begin_kernel_us": begin_c,
                      "b_plain_after_steps_ms": med(t_b2), "d_keep_played_ms": med(t_d), "d_begin_kernel_us": begin_d,
                      "d_rows_kept_share": round(float(np.mean(kept_share)), 4), "d_mean_carried_visits": round(float(np.mean(visits)), 3),
                      "d_mean_carried_nodes": round(float(np.mean(nodes)), 2), "d_pool_full_rows": full,
                      "reps_ms": {"b": [round(x, 3) for x in t_b], "c": [round(x, 3) for x in t_c], "b_after_steps": [round(x, 3) for x in t_b2],
                                  "d": [round(x, 3) for x in t_d]}}), flush=True)
    b.close()


def _child(a, mode, root):
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", mode, "--root", root, "--envs", str(a.envs),
           "--settle", str(a.settle), "--reps", str(a.reps), "--waves", str(a.waves), "--par", str(a.par)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    lines = [json.loads(s) for s in r.stdout.splitlines() if s.startswith("{")]
    if r.returncode != 0 or not lines:
        print(json.dumps({"error": f"{mode} in {root}: exit status {r.returncode}", "stderr": r.stderr[-2000:]}), flush=True)
        sys.exit(1)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="", help="a checkout of the parent commit with its library built (none: (a) is left out)")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--settle", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--waves", type=int, default=8)
    ap.add_argument("--par", type=int, default=8)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "tree_keep_ab.json"))
    ap.add_argument("--child", default="")
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        (run_plain if a.child == "plain" else run_keep)(os.path.abspath(a.root), a.envs, a.settle, a.reps, a.waves, a.par)
        return
    rec = {"tool": "tools/tree_keep_ab.py", "envs": a.envs}
    order = [("a", os.path.abspath(a.parent)), ("b", ROOT)] * 2 if a.parent else [("b", ROOT)]
    runs = {"a": [], "b": []}
    digests = set()
    for which, root in order:                  # parent, this commit, parent, this commit: each a process of its own
        line = _child(a, "plain", root)[-1]
        runs[which] += line["plain_ms"]
        digests.add(line["digest"])
    if a.parent:
        lo, hi = min(runs["a"]), max(runs["a"])
        import statistics
        med_b = statistics.median(runs["b"])
        rec.update(a_parent_plain_ms=runs["a"], a_range_ms=[lo, hi], b_this_commit_plain_ms=runs["b"], b_median_ms=round(med_b, 3),
                   a_median_ms=round(statistics.median(runs["a"]), 3), b_inside_a_range_widened_by_its_width=bool(lo - (hi - lo) <= med_b <= hi + (hi - lo)),
                   plain_search_results_equal_across_builds=len(digests) == 1)
    else:
        rec.update(b_this_commit_plain_ms=runs["b"])
    keep = [l for l in _child(a, "keep", ROOT) if "b_plain_ms" in l][-1]
    rec.update(keep)
    lo, hi = min(keep["reps_ms"]["b"]), max(keep["reps_ms"]["b"])
    rec["c_inside_b_range_widened_by_its_width"] = bool(lo - (hi - lo) <= keep["c_keep_fresh_ms"] <= hi + (hi - lo))
    with open(a.json, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in rec.items() if k != "reps_ms"}), flush=True)


if __name__ == "__main__":
    main()
