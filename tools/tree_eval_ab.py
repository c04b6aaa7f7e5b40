#!/usr/bin/env python3
"""What a wave of the evaluated tree search costs beside a wave of the rollout search (XR-Tree v1), on the ispd18_test1 pack at the
stationary nets-left distribution, HIP events, every shape warmed up first, repetitions alternated:

  (a) per wave of the evaluated search at rows x n_par: select + peek (`tree_leaves`), expand + tower + critic + actor head (the
      evaluator), backup (`tree_backup`) — each timed on its own inside running sessions, and the whole session over its waves;
  (b) per wave of `tree_search` (select + rollout + backup) at the same rows x n_par: a search of the same number of waves over its
      waves (the reset launch included, as (a) includes the open call);
  (c) nets routed per simulation in both forms: the mean path length of (a)'s simulations, the mean nets left per live env for (b)
      (a v1 simulation routes them all);
  (d) episode returns of `tree_episodes` and `evaluated_episodes` at equal simulations per ply on the first --episode-regions regions.
THE NETWORK IS UNTRAINED (a seeded ActorCritic): the returns of (d) are recorded, not judged.

    python tools/tree_eval_ab.py [--envs 1024] [--waves 4] [--par 4] [--json profiles/tree_eval_ab.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 977
sys.path.insert(0, ROOT)


def _timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--settle", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--waves", type=int, default=4)
    ap.add_argument("--par", type=int, default=4)
    ap.add_argument("--episode-regions", type=int, default=32)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "tree_eval_ab.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from xroute_env_amd.agents import ActorCritic, GroupedFusedPolicy
    from xroute_env_amd.batch import RegionBatch
    from xroute_env_amd.envs import peek as pk
    from xroute_env_amd.envs.tree import tree_episodes
    from xroute_env_amd.envs.tree_eval import actor_critic_evaluator, evaluated_episodes, evaluated_search
    from xroute_env_amd.lefdef import load_region_pack
    if not torch.cuda.is_available():
        raise SystemExit("tools/tree_eval_ab.py measures on the GPU: no device here, nothing measured")
    DEV = "cuda:0"
    regions = load_region_pack(os.path.join(ROOT, "tests", "golden", "ispd18_test1_regions.npz"))
    n, W, P = a.envs, a.waves, a.par
    b = RegionBatch(regions, n_envs=n, device=DEV, auto_reset=True)
    b.reset()
    act = torch.empty(n, dtype=torch.int32, device=DEV)
    for s in range(a.settle):                    # to the stationary nets-left distribution
        b.step(b.random_actions(SEED + s, act))
    torch.manual_seed(7)
    model = ActorCritic(device=DEV).to(DEV).eval()
    pol = GroupedFusedPolicy(model, b)
    groups = pk.shape_groups(b)
    evaluate = actor_critic_evaluator(model, pol, groups)
    K = max(b.k_max, 1)
    cap = 1 + (W * P + 1) * K
    v1 = lambda: b.tree_search(W, P, SEED, node_cap=cap)
    v2 = lambda: evaluated_search(b, evaluate, W, P, node_cap=cap, trace=True)
    for _ in range(2):                           # every shape of the timed windows, warmed up
        v1(); v2()
    torch.cuda.synchronize()
    t_v1, t_v2, t_leaves, t_eval, t_backup, depth = [], [], [], [], [], []
    for _ in range(a.reps):                      # alternated
        t_v1.append(_timed(torch, v1)[0] / W)
        ms, res = _timed(torch, v2)
        t_v2.append(ms / W)
        live = b.fetch("nlegal") > 0
        depth.append(float((res["paths"][live] > 0).sum(dim=2).to(torch.float64).mean()))
        b.tree_open(P, W * P, None, cap)         # the stages, each on its own, inside a running session
        tl = te = tb = 0.0
        for w in range(W):
            ms, lv = _timed(torch, lambda: b.tree_leaves()); tl += ms
            ms, (value, prior) = _timed(torch, lambda: evaluate(b, lv)); te += ms
            ms, _ = _timed(torch, lambda: b.tree_backup(value, prior)); tb += ms
        t_leaves.append(tl / W); t_eval.append(te / W); t_backup.append(tb / W)
    nl = b.fetch("nlegal")
    live = nl > 0
    med = lambda t: round(float(np.median(t)), 4)
    rec = {"tool": "tools/tree_eval_ab.py", "command": " ".join([os.path.basename(sys.executable)] + sys.argv), "device": torch.cuda.get_device_name(0),
           "envs": n, "live_envs": int(live.sum()), "n_waves": W, "n_par": P, "node_cap": cap, "k_max": K, "reps": a.reps,
           "network": "ActorCritic, torch.manual_seed(7), UNTRAINED",
           "fused_towers": int(sum(t is not None for t in pol.towers)), "grid_shapes": len(pol.shapes),
           "a_evaluated_wave_ms": med(t_v2), "a_select_peek_ms": med(t_leaves), "a_expand_tower_critic_actor_ms": med(t_eval), "a_backup_ms": med(t_backup),
           "b_v1_wave_ms": med(t_v1),
           "c_nets_routed_per_simulation": {"evaluated": round(float(np.mean(depth)), 3), "v1": round(float(nl[live].to(torch.float64).mean()), 3)},
           "reps_ms": {"a_wave": [round(x, 4) for x in t_v2], "b_wave": [round(x, 4) for x in t_v1], "a_select_peek": [round(x, 4) for x in t_leaves],
                       "a_evaluator": [round(x, 4) for x in t_eval], "a_backup": [round(x, 4) for x in t_backup]}}
    b.close()
    # (d) whole episodes at equal simulations per ply; the network is untrained: recorded, not judged
    sub = regions[:a.episode_regions]
    s1, s2 = {}, {}
    e1 = tree_episodes(sub, W, P, seed=SEED, device=DEV, stats=s1)
    e2 = evaluated_episodes(sub, actor_critic_evaluator(model), W, P, device=DEV, stats=s2)
    rec["d_episodes"] = {"regions": len(sub), "simulations_per_ply": W * P,
                         "v1_mean_return": round(float(np.mean([o["ret"] for o in e1])), 4), "evaluated_mean_return": round(float(np.mean([o["ret"] for o in e2])), 4),
                         "v1_routed_nets": s1["routed_nets"], "evaluated_routed_nets": s2["routed_nets"], "judged": False}
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in rec.items() if k != "reps_ms"}), flush=True)


if __name__ == "__main__":
    main()
