#!/usr/bin/env python3
"""A tree search whose leaves a network values, on the regions of ispd18_test1: the evaluated tree search (RegionBatch.tree_open /
tree_leaves / tree_backup, `envs.tree_eval`) beside the orderings the project already had.  Four orderings are compared —

  random           a random legal net per ply;
  greedy           the net of the highest one-step reward (lookahead);
  tree (v1)        the rollout search: every simulation plays the episode to its end at random, the most visited net is stepped;
  evaluated tree   every simulation stops at its leaf: the leaf's state goes through the obstacle tower, the critic values it and the
                   actor's softmax is the prior of its children (`envs.tree_eval.actor_critic_evaluator`), the most visited net is stepped.

THE NETWORK IS UNTRAINED: a seeded, randomly initialised ActorCritic.  Its values and priors carry no information about routing cost,
so the evaluated-tree row says nothing about what a trained network would do — this example shows the plumbing (per wave: select, peek,
expand, tower + critic + actor head, backup, all enqueue-only), not a result.

With --reuse the evaluated tree is also played with tree reuse ("XR-Tree v2, kept": `envs.tree_eval.evaluated_episodes(reuse=True)`,
RegionBatch.tree_open(keep=True, played=...)): the session of a ply continues from the subtree below the net just stepped.  Beside the
fresh episodes it prints the visits and nodes the kept trees carried per ply and the nets the simulations routed.  The network is the
same UNTRAINED one: these numbers, too, show plumbing, not quality.

    python examples/network_tree.py [regions=64] [waves=4] [lanes=4] [--reuse]
"""
import argparse
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from xroute_env_amd.agents import ActorCritic, GroupedFusedPolicy
from xroute_env_amd.envs import peek as pk
from xroute_env_amd.envs.tree_eval import actor_critic_evaluator, evaluated_episodes, evaluated_search
from xroute_env_amd.envs.vector_env import XRouteVectorEnv
from xroute_env_amd.lefdef import load_region_pack

ap = argparse.ArgumentParser()
ap.add_argument("regions", nargs="?", type=int, default=64)
ap.add_argument("waves", nargs="?", type=int, default=4)
ap.add_argument("lanes", nargs="?", type=int, default=4)
ap.add_argument("--reuse", action="store_true", help="also play the evaluated tree with tree reuse (XR-Tree v2, kept)")
a = ap.parse_args()
pack = load_region_pack(os.path.join(ROOT, "tests", "golden", "ispd18_test1_regions.npz"))[:a.regions]
R = len(pack)
DEV = "cuda:0"
torch.manual_seed(7)
model = ActorCritic(device=DEV).to(DEV).eval()
print("network: ActorCritic with torch.manual_seed(7), UNTRAINED — the evaluated-tree row below shows the plumbing, not a trained network's quality")


def play(policy):
    """One episode of every region (slot r plays region r; a slot's first `done` ends what is counted for it)."""
    env = XRouteVectorEnv(pack, n_envs=R, device=DEV, with_observation=False)
    env.batch.assign(list(range(R)))
    env.batch.reset()
    evaluate = None
    if policy == "evaluated":
        groups = pk.shape_groups(env.batch)          # (the slots keep their regions for the episode: one host round trip, here)
        evaluate = actor_critic_evaluator(model, GroupedFusedPolicy(model, env.batch), groups)
    ret = torch.zeros(R, dtype=torch.float64, device=env.device)
    live = torch.ones(R, dtype=torch.bool, device=env.device)
    routed = 0
    for t in range(env.kmax + 1):
        if policy == "greedy":
            actions = env.greedy_actions()
        elif policy == "random":
            actions = env.random_actions(1234 + t)
        elif policy == "tree":
            routed += a.waves * a.lanes * int(env.batch.fetch("nlegal").sum())
            actions = env.tree_actions(a.waves, a.lanes, 1234 + t)
        else:
            res = evaluated_search(env.batch, evaluate, a.waves, a.lanes, trace=True)
            routed += int((res["paths"] > 0).sum())
            actions = XRouteVectorEnv._most_visited(res)
        _, reward, done, _ = env.step(actions)
        ret += torch.where(live, reward, torch.zeros_like(reward))
        live &= ~done.bool()
        if not bool(live.any()):
            break
    return -float(ret.mean()), routed


for policy, name in (("random", "random"), ("greedy", "greedy"), ("tree", "tree (v1) %d x %d, random rollouts" % (a.waves, a.lanes)),
                     ("evaluated", "evaluated tree %d x %d (untrained)" % (a.waves, a.lanes))):
    cost, routed = play(policy)
    extra = f", {routed} nets routed by its simulations" if routed else ""
    print(f"{name:40s} ordering: mean episode cost {cost:.1f} over {R} regions{extra}")

if a.reuse:
    print("tree reuse (UNTRAINED network: plumbing, not quality) — episodes of evaluated_episodes, fresh sessions beside reopened ones:")
    for reuse in (False, True):
        stats = {}
        out = evaluated_episodes(pack, actor_critic_evaluator(model), a.waves, a.lanes, device=DEV, stats=stats, reuse=reuse)
        cost = -sum(o["ret"] for o in out) / len(out)
        line = f"{'reopened' if reuse else 'fresh':10s} sessions: mean episode cost {cost:.1f}, {stats['routed_nets']} nets routed by the simulations of {stats['plies']} plies"
        if reuse:
            line += f", carried per ply {stats['carried_visits'] / stats['plies']:.2f} visits and {stats['carried_nodes'] / stats['plies']:.2f} nodes"
        print(line)
