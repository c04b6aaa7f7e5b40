#!/usr/bin/env python3
"""What peek costs (xr_batch_peek), on the 4096-slot ispd18_test1 pack at the stationary nets-left distribution, every successor of
every env peeked with envs.peek.successor_prefix; HIP events, warm-up first, 7 repetitions, legs alternated:

  (i)   peek + expand_state of every row (in chunks of envs, into one head buffer): per call and per successor;
  (ii)  the same heads without peek: state_dict, then per candidate rank c a step_compact with every env's rank-c candidate, a copy of
        the head, load_state_dict — k_max rounds.  First asserted to give (i)'s heads byte for byte.  The ratio is reported; none was
        fixed in advance;
  (iii) rollout(policy="stop") with the same prefix: what packing adds to a route-only line.  Yardstick: (i)'s peek alone must lie
        inside (iii)'s min-max range widened by that range's own width;
  (iv)  xr_batch_rollout with the random policy on a checkout of the PARENT commit (--parent-root: a tree with its own built library)
        and on this tree, each in a process of its own, alternated: this tree's median must lie inside the parent's widened range;
  (v)   envs.peek.successor_values end to end with a seeded, untrained ActorCritic, and its split into peek, expand and tower + critic.

One child process per measurement under a `timeout`; nothing is started after a failure.

    python tools/peek_ab.py [--parent-root DIR] [--envs 4096] [--json profiles/peek_ab.json]
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


def settled_batch(root, n, settle):
    """The package of `root`; (regions, a batch of n slots stepped to the stationary nets-left distribution)."""
    sys.path.insert(0, root)
    import torch
    from xroute_env_amd.batch import RegionBatch
    from xroute_env_amd.lefdef import load_region_pack
    regions = load_region_pack(os.path.join(HERE, "tests", "golden", "ispd18_test1_regions.npz"))
    dev = "cuda:0"
    b = RegionBatch(regions, n_envs=n, device=dev, auto_reset=True)
    b.reset()
    act = torch.empty(n, dtype=torch.int32, device=dev)
    for s in range(settle):
        b.step(b.random_actions(SEED + s, act))
    return regions, b


def run_rollout(root, n, settle, reps, R=16):
    """(iv): the existing rollout kernel, which every tree can run."""
    import torch
    _, b = settled_batch(root, n, settle)
    nl = b.fetch("nlegal").cpu().numpy()
    ra = b.rollout(R, SEED)
    roll = lambda: b.rollout(R, SEED, out=ra["out"], return_out=ra["ret"], hash_out=ra["hash"], order_out=ra["order"])
    for _ in range(2):
        roll()
    torch.cuda.synchronize()
    print(json.dumps({"envs": n, "rollouts": R, "rollout_routes": int(nl.sum()) * R, "random_ms": [round(timed_once(roll), 3) for _ in range(reps)]}), flush=True)
    return True


def run_peek(root, n, settle, reps, chunk, ii_reps):
    import torch
    regions, b = settled_batch(root, n, settle)
    from xroute_env_amd.agents import ActorCritic, FusedObstacleTower
    from xroute_env_amd.batch import RegionBatch
    from xroute_env_amd.envs import peek as pk
    dev = b.device
    # the same state in a batch with auto_reset off: a step with action 0 is a no-op there, for done envs too (leg (ii) needs that)
    w = RegionBatch(regions, n_envs=n, device=dev, auto_reset=False)
    w.reset()
    w.load_state_dict(b.state_dict())
    b.close()
    K, W, rb = w.k_max, 2 * w.n_max, w.state_row_bytes()
    nl = w.fetch("nlegal").cpu().numpy()
    prefix = pk.successor_prefix(w)
    res = w.peek(prefix)
    bufs = dict(rows_out=res["rows"], out=res["out"], return_out=res["ret"], hash_out=res["hash"], order_out=res["order"])
    head = torch.empty((chunk * K, W), dtype=torch.float32, device=dev)
    nlo, rgo = torch.empty(chunk * K, dtype=torch.int32, device=dev), torch.empty(chunk * K, dtype=torch.int32, device=dev)

    def expand_all(keep=None):
        for lo in range(0, n, chunk):
            hi = min(n, lo + chunk)
            m = (hi - lo) * K
            w.expand_state(res["rows"][lo:hi].reshape(m, rb), head[:m], nlo[:m], rgo[:m])
            if keep is not None:
                keep(lo, hi, head[:m].view(hi - lo, K, W))

    # ---- (ii) and the identity of the heads ---------------------------------------------------------------------------------------
    heads_ii = torch.empty((K, n, W), dtype=torch.float32, device=dev)          # (K x n x 2 n_max floats: room a 288 GB card has)
    head_step = w.alloc_head()
    cand = prefix[:, :, 0].t().contiguous()                                     # [K, n]: every env's rank-c candidate (0: none, a no-op)

    def without_peek():
        sd = w.state_dict()
        for c in range(K):
            w.step_compact(cand[c], head_step)
            heads_ii[c].copy_(head_step)
            w.load_state_dict(sd)

    without_peek()
    reg = w.fetch("region").cpu().numpy()
    n2 = torch.tensor([2 * regions[int(r)].n_nodes for r in reg], device=dev)
    in_head = torch.arange(W, device=dev)[None, :] < n2[:, None]                # the 2 N floats of every env's own region
    same = []

    def compare(lo, hi, h):
        ref = heads_ii[:, lo:hi].permute(1, 0, 2)
        mask = in_head[lo:hi, None, :].expand(hi - lo, K, W)
        same.append(bool(torch.equal(h.view(torch.int32)[mask], ref.contiguous().view(torch.int32)[mask])))

    w.peek(prefix, **bufs)
    expand_all(compare)
    torch.cuda.synchronize()
    assert same and all(same), "peek + expand_state and the state_dict / step_compact / load_state_dict loop give different heads"
    assert torch.equal(w.fetch("nlegal").cpu(), torch.from_numpy(nl)), "leg (ii) did not restore the batch"

    # ---- (i) and (iii), alternated ------------------------------------------------------------------------------------------------
    ro = w.rollout(K, 0, policy="stop", prefix=prefix)
    robufs = dict(out=ro["out"], return_out=ro["ret"], hash_out=ro["hash"], order_out=ro["order"])
    peek = lambda: w.peek(prefix, **bufs)
    stop = lambda: w.rollout(K, 0, policy="stop", prefix=prefix, **robufs)
    assert all(torch.equal(res[k], ro[k]) for k in ("out", "hash", "order")), "peek's record differs from rollout(policy='stop')"
    for _ in range(2):
        peek(); stop(); expand_all()
    t_peek, t_stop, t_expand = [], [], []
    for i in range(reps):
        for which in ((0, 1) if i % 2 == 0 else (1, 0)):
            (t_stop if which else t_peek).append(timed_once(stop if which else peek))
        t_expand.append(timed_once(expand_all))
    # where packing's time goes: the same pair on lines that all route (one line per env, its first candidate) and on lines that
    # never do (no prefix, k_max lines per env: the shadow load and the record in both kernels, the pack pass in peek only)
    first = prefix[:, :1].contiguous()
    split = {}
    for name, pfx, L in (("dense", first, 1), ("empty", None, K)):
        rp, rr = w.peek(pfx, n_lines=L), w.rollout(L, 0, policy="stop", prefix=pfx)
        pb = dict(rows_out=rp["rows"], out=rp["out"], return_out=rp["ret"], hash_out=rp["hash"], order_out=rp["order"])
        sb = dict(out=rr["out"], return_out=rr["ret"], hash_out=rr["hash"], order_out=rr["order"])
        pk_, st_ = (lambda: w.peek(pfx, n_lines=L, **pb)), (lambda: w.rollout(L, 0, policy="stop", prefix=pfx, **sb))
        for _ in range(2):
            pk_(); st_()
        tp, ts = [], []
        for i in range(reps):
            for which in ((0, 1) if i % 2 == 0 else (1, 0)):
                (ts if which else tp).append(timed_once(st_ if which else pk_))
        split[name] = {"lines": n * L, "peek_ms": [round(t, 3) for t in tp], "stop_rollout_ms": [round(t, 3) for t in ts]}
    t_ii = [timed_once(without_peek) for _ in range(ii_reps)]          # (host round trips, k_max of them)

    # ---- (v) successor_values end to end ------------------------------------------------------------------------------------------
    torch.manual_seed(7)
    model = ActorCritic(device=dev).to(dev).eval()                              # seeded, UNTRAINED: the plumbing, not the quality
    shapes = sorted({tuple(int(v) for v in r.dims) for r in regions})
    towers = {s: FusedObstacleTower(model.representation_network, (s[2], s[1], s[0]), dev) for s in shapes}
    groups = [(d, torch.arange(n, device=dev) if i is None else i) for d, i in pk.shape_groups(w)]
    values = lambda: pk.successor_values(model, w, towers, chunk=chunk, groups=groups)

    def tower_critic_only():          # the third part alone, on whatever the head buffer holds, in successor_values' pieces
        for dims, idx in groups:
            for lo in range(0, int(idx.numel()), chunk):
                m = min(chunk, int(idx.numel()) - lo) * K
                pk.state_values(model, head[:m], dims, towers)

    for _ in range(2):
        values(); tower_critic_only()
    t_values = [timed_once(values) for _ in range(reps)]
    t_tower = [timed_once(tower_critic_only) for _ in range(reps)]
    r3 = lambda v: [round(t, 3) for t in v]
    print(json.dumps({"envs": n, "k_max": K, "n_max": w.n_max, "row_bytes": rb, "chunk": chunk, "successors": int(nl.sum()), "lines": n * K,
                      "mean_nets_left": round(float(nl.mean()), 3), "same_heads": True, "shapes": len(shapes),
                      "fused_tower_shapes": sum(1 for t in towers.values() if t.supported),
                      "peek_ms": r3(t_peek), "expand_ms": r3(t_expand), "stop_rollout_ms": r3(t_stop), "without_peek_ms": r3(t_ii),
                      "successor_values_ms": r3(t_values), "tower_critic_ms": r3(t_tower), "split": split}), flush=True)
    return True


def inside(x, ref):
    """x inside ref's min-max range widened by that range's own width."""
    lo, hi = min(ref), max(ref)
    return lo - (hi - lo) <= x <= hi + (hi - lo)


def child(root, a, what):
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", what, "--root", root, "--envs", str(a.envs),
           "--settle", str(a.settle), "--reps", str(a.reps), "--chunk", str(a.chunk), "--ii-reps", str(a.ii_reps)]
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
    ap.add_argument("--settle", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ii-reps", type=int, default=7, help="repetitions of leg (ii), the slow one")
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built: measures (iv)")
    ap.add_argument("--json", default=os.path.join(HERE, "profiles", "peek_ab.json"))
    ap.add_argument("--child", default=None, choices=("peek", "rollout"))
    ap.add_argument("--root", default=HERE)
    a = ap.parse_args()
    if a.child:
        fn = run_peek if a.child == "peek" else run_rollout
        sys.exit(0 if fn(a.root, a.envs, a.settle, a.reps, *((a.chunk, a.ii_reps) if a.child == "peek" else ())) else 1)
    med = lambda v: sorted(v)[len(v) // 2]
    p = child(HERE, a, "peek")
    m = {k: med(p[k]) for k in ("peek_ms", "expand_ms", "stop_rollout_ms", "without_peek_ms", "successor_values_ms", "tower_critic_ms")}
    i_ms = m["peek_ms"] + m["expand_ms"]
    rec = {"tool": "tools/peek_ab.py", **{k: p[k] for k in ("envs", "k_max", "n_max", "row_bytes", "chunk", "successors", "lines", "mean_nets_left",
                                                             "same_heads", "shapes", "fused_tower_shapes")},
           "i_peek_ms": p["peek_ms"], "i_expand_ms": p["expand_ms"], "i_peek_median_ms": m["peek_ms"], "i_expand_median_ms": m["expand_ms"],
           "i_median_ms": round(i_ms, 3), "i_us_per_successor": round(1e3 * i_ms / max(1, p["successors"]), 3),
           "i_peek_us_per_successor": round(1e3 * m["peek_ms"] / max(1, p["successors"]), 3),
           "ii_without_peek_ms": p["without_peek_ms"], "ii_median_ms": m["without_peek_ms"], "ii_over_i": round(m["without_peek_ms"] / i_ms, 2),
           "iii_stop_rollout_ms": p["stop_rollout_ms"], "iii_median_ms": m["stop_rollout_ms"],
           "peek_over_stop_rollout": round(m["peek_ms"] / m["stop_rollout_ms"], 4),
           "peek_inside_stop_rollout_range_widened_by_its_width": inside(m["peek_ms"], p["stop_rollout_ms"]),
           "iii_split": {k: dict(v, peek_median_ms=med(v["peek_ms"]), stop_median_ms=med(v["stop_rollout_ms"]),
                                 peek_over_stop=round(med(v["peek_ms"]) / med(v["stop_rollout_ms"]), 4)) for k, v in p["split"].items()},
           "v_successor_values_ms": p["successor_values_ms"], "v_median_ms": m["successor_values_ms"],
           "v_tower_critic_ms": p["tower_critic_ms"], "v_split_median_ms": {"peek": m["peek_ms"], "expand": m["expand_ms"], "tower_critic": m["tower_critic_ms"]},
           "v_model": "ActorCritic, torch.manual_seed(7), untrained"}
    if a.parent_root:
        par, new = [], []
        for i in range(2):                     # two processes per tree, alternated
            for which in ((0, 1) if i == 0 else (1, 0)):
                r = child(os.path.abspath(a.parent_root) if which == 0 else HERE, a, "rollout")
                (par if which == 0 else new).append(r)
        assert len({r["rollout_routes"] for r in par + new}) == 1, "the trees' batches are in different states"
        pm, nm = sum((r["random_ms"] for r in par), []), sum((r["random_ms"] for r in new), [])
        rec.update(iv_parent_random_rollout_ms=pm, iv_this_random_rollout_ms=nm, iv_parent_median_ms=med(pm), iv_this_median_ms=med(nm),
                   iv_this_over_parent=round(med(nm) / med(pm), 4), iv_this_inside_parent_range_widened_by_its_width=inside(med(nm), pm))
    else:
        rec.update(iv_parent_random_rollout_ms=None, note="(iv) not measured: no --parent-root")
    print(json.dumps(rec), flush=True)
    with open(a.json, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
