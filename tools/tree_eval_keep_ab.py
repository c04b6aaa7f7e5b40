#!/usr/bin/env python3
"""What tree reuse costs and carries in the evaluated search (xr_batch_tree_reopen, "XR-Tree v2, kept"), on the 4096-slot ispd18_test1
pack at the stationary nets-left distribution, 8 waves x 8 lanes, a synthetic evaluator (a hash of the leaf's packed row: the search is
timed, not a network), HIP events, warm-up first, 7 repetitions, variants alternated within a process:

  (a) a plain open session (tree_open, then per wave leaves -> evaluator -> backup) on a build of the PARENT commit (--parent DIR: a
      checkout of the parent with its library built; a process of its own, run before and after this commit's), against
  (b) the same session on this commit: its median must lie inside (a)'s own min-max range widened by that range's width on either side;
  (c) the session started by reopen with played = None, alternated with (b): (a), (b) and (c) must give the same session (a digest of
      the last wave's visits, nodes_used and returns);
  (d) at the states after each of 7 real steps (the most visited nets of the reopened session), a fresh open session beside a reopen
      with the actions stepped: both times, the share of live rows kept, the mean visits and nodes carried, the mean path length of the
      simulations fresh against kept (deeper paths are more routes per evaluated simulation), rows that hit XR_TREE_POOL_FULL.  The fresh
      session runs as env group 0 of a one-group split — the same rows through the same kernels, on the group's own pool — because an
      open session on the whole batch's pool would end the keyed one.
The reopen kernel on its own comes from the kernel records of torch.profiler (null where it gives none).  Nothing is promised for (d).
Child processes under a `timeout`; nothing is started after a failure.

    python tools/tree_eval_keep_ab.py [--parent DIR] [--envs 4096] [--json profiles/tree_eval_keep_ab.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 977


def _setup(root, n, settle, groups=False):
    sys.path.insert(0, root)
    import torch
    from xroute_env_amd.batch import RegionBatch
    from xroute_env_amd.lefdef import load_region_pack
    regions = load_region_pack(os.path.join(ROOT, "tests", "golden", "ispd18_test1_regions.npz"))
    b = RegionBatch(regions, n_envs=n, device="cuda:0", auto_reset=True)
    if groups:
        b.set_groups([0, n])
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


def _session(torch, b, n_waves, opener, group=None):
    """One session: opener() starts it, then n_waves x (leaves, the synthetic evaluator, backup).  (last result, kept, the waves' paths)."""
    kept = opener()
    paths, res = [], None
    for _ in range(n_waves):
        lv = b.tree_leaves(group=group)
        rows = lv["rows"]
        wt = (torch.arange(rows.shape[-1], device=rows.device, dtype=torch.int64) * 2654435761 + 12345) % 1000003 + 1
        h = (rows.to(torch.int64) * wt).sum(-1) % 1000003
        value = ((h.to(torch.float64) / 1000003.0 - 0.7) * 3.1).contiguous()
        res = b.tree_backup(value, None, group=group)
        paths.append(lv["paths"])
    return res, kept, paths


def _digest(torch, res):
    return int(res["visits"].to(torch.int64).sum()) * 1000003 + int(res["info"][:, 1].to(torch.int64).sum()) * 101 + int((res["returns"] * 1e6).to(torch.int64).sum() % 1000003)


def run_plain(root, n, settle, reps, n_waves, n_par):
    torch, b = _setup(root, n, settle)
    S = n_waves * n_par
    cap = 1 + (S + 1) * max(b.k_max, 1)
    fn = lambda: _session(torch, b, n_waves, lambda: b.tree_open(n_par, S, None, cap))
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t = [_timed(torch, fn)[0] for _ in range(reps)]
    print(json.dumps({"plain_ms": [round(x, 3) for x in t], "digest": _digest(torch, fn()[0]), "library": os.path.join(root, "xroute_env_amd")}), flush=True)
    b.close()


def _reopen_kernel_us(torch, fn):
    """The device time of xr_tree_eval_reopen_kernel in one call of fn, from torch.profiler's kernel records (None: no such record)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        for ev in prof.events():
            if "xr_tree_eval_reopen_kernel" in ev.name:
                us = getattr(ev, "device_time", None)
                return float(us if us is not None else ev.cuda_time)
    except Exception as exc:          # the measurement is optional: say why it is missing
        print(json.dumps({"profiler": repr(exc)[:300]}), flush=True)
    return None


def run_keep(root, n, settle, reps, n_waves, n_par):
    import numpy as np
    torch, b = _setup(root, n, settle, groups=True)
    from xroute_env_amd import _lib
    from xroute_env_amd.envs.vector_env import XRouteVectorEnv
    K, S = max(b.k_max, 1), n_waves * n_par
    cap1 = 1 + (S + 1) * K
    cap = 1 + 2 * (S + 1) * K
    plain = lambda: _session(torch, b, n_waves, lambda: b.tree_open(n_par, S, None, cap1))
    fresh = lambda: _session(torch, b, n_waves, lambda: b.tree_open(n_par, S, None, cap1, keep=True))
    for _ in range(2):
        plain(); fresh()
    torch.cuda.synchronize()
    d_b, d_c = _digest(torch, plain()[0]), _digest(torch, fresh()[0])
    t_b, t_c = [], []
    for _ in range(reps):                      # alternated
        t_b.append(_timed(torch, plain)[0])
        t_c.append(_timed(torch, fresh)[0])
    kernel_c = _reopen_kernel_us(torch, lambda: b.tree_open(n_par, S, None, cap1, keep=True))
    # (d): search, step the most visited net, reopen — every repetition is the session after one more real step
    open_g = lambda: _session(torch, b, n_waves, lambda: b.tree_open(n_par, S, None, cap, group=0), group=0)
    res, _, _ = _session(torch, b, n_waves, lambda: b.tree_open(n_par, S, None, cap, keep=True))
    open_g()
    t_f, t_d, share, visits, nodes, len_f, len_d, kernel_d, full = [], [], [], [], [], [], [], None, 0
    depth = lambda paths, live: float(torch.stack([(p[live] > 0).sum(dim=2).to(torch.float64).mean() for p in paths]).mean())
    for r in range(reps + 2):
        act = XRouteVectorEnv._most_visited(res)
        b.step(act)
        live = b.fetch("nlegal") > 0
        reopen = lambda: _session(torch, b, n_waves, lambda: b.tree_open(n_par, S, None, cap, keep=True, played=act))
        if r == 0:                             # (one unmeasured round: the continued session's first)
            res = reopen()[0]
            continue
        if r == reps + 1:                      # (and one under the profiler, for the first kernel alone)
            kernel_d = _reopen_kernel_us(torch, lambda: b.tree_open(n_par, S, None, cap, keep=True, played=act))
            break
        ms, (_, _, pf) = _timed(torch, open_g)
        t_f.append(ms)
        ms, (res, kept, pd) = _timed(torch, reopen)
        t_d.append(ms)
        k = kept[live].to(torch.float64)
        share.append(float(((res["info"][live, 3] & _lib.XR_TREE_KEPT) != 0).to(torch.float64).mean()))
        visits.append(float(k[:, 0].mean())); nodes.append(float(k[:, 1].mean()))
        len_f.append(depth(pf, live)); len_d.append(depth(pd, live))
        full += int(((res["info"][:, 3] & _lib.XR_TREE_POOL_FULL) != 0).sum())
    med = lambda t: round(float(np.median(t)), 3)
    print(json.dumps({"n_waves": n_waves, "n_par": n_par, "node_cap_open": cap1, "node_cap_keyed": cap, "k_max": K, "digest_b": d_b, "digest_c": d_c,
                      "b_open_ms": med(t_b), "c_reopen_fresh_ms": med(t_c), "c_reopen_kernel_us": kernel_c,
                      "d_fresh_open_after_steps_ms": med(t_f), "d_reopen_played_ms": med(t_d), "d_reopen_kernel_us": kernel_d,
                      "d_rows_kept_share": round(float(np.mean(share)), 4), "d_mean_carried_visits": round(float(np.mean(visits)), 3),
                      "d_mean_carried_nodes": round(float(np.mean(nodes)), 2), "d_mean_path_length_fresh": round(float(np.mean(len_f)), 3),
                      "d_mean_path_length_kept": round(float(np.mean(len_d)), 3), "d_pool_full_rows": full,
                      "reps_ms": {"b": [round(x, 3) for x in t_b], "c": [round(x, 3) for x in t_c], "d_fresh": [round(x, 3) for x in t_f],
                                  "d_reopen": [round(x, 3) for x in t_d]}}), flush=True)
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
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "tree_eval_keep_ab.json"))
    ap.add_argument("--child", default="")
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        (run_plain if a.child == "plain" else run_keep)(os.path.abspath(a.root), a.envs, a.settle, a.reps, a.waves, a.par)
        return
    rec = {"tool": "tools/tree_eval_keep_ab.py", "envs": a.envs, "evaluator": "synthetic: a hash of the leaf's packed row"}
    order = [("a", os.path.abspath(a.parent)), ("b", ROOT)] * 2 if a.parent else [("b", ROOT)]
    runs = {"a": [], "b": []}
    digests = set()
    for which, root in order:                  # parent, this commit, parent, this commit: each a process of its own
        line = _child(a, "plain", root)[-1]
        runs[which] += line["plain_ms"]
        digests.add(line["digest"])
    if a.parent:
        lo, hi = min(runs["a"]), max(runs["a"])
        med_b = statistics.median(runs["b"])
        rec.update(a_parent_open_ms=runs["a"], a_range_ms=[lo, hi], b_this_commit_open_ms=runs["b"], b_median_ms=round(med_b, 3),
                   a_median_ms=round(statistics.median(runs["a"]), 3), b_inside_a_range_widened_by_its_width=bool(lo - (hi - lo) <= med_b <= hi + (hi - lo)))
    else:
        rec.update(b_this_commit_open_ms=runs["b"])
    keep = [l for l in _child(a, "keep", ROOT) if "b_open_ms" in l][-1]
    digests.update((keep["digest_b"], keep["digest_c"]))
    rec.update(keep)
    rec["a_b_c_give_the_same_session"] = len(digests) == 1
    with open(a.json, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in rec.items() if k != "reps_ms"}), flush=True)
    if not rec["a_b_c_give_the_same_session"] or not rec.get("b_inside_a_range_widened_by_its_width", True):
        sys.exit(2)


if __name__ == "__main__":
    main()
