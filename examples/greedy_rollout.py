#!/usr/bin/env python3
"""The greedy net ordering — the cost baseline a learned ordering is meant to beat: at every step each env routes the net whose route is
cheapest NOW (`XRouteVectorEnv.greedy_actions`: the arg-max of the lookahead rewards, every candidate net of every env priced on the
device without stepping) — beside the built-in random ordering, on the regions of ispd18_test1.  Whole-batch rollout; prints the mean
episode cost (violations x 500 + vias x 4 + wirelength x 0.5, the trainers' reward negated) of both policies over the same regions.

    python examples/greedy_rollout.py [slots=1024] [steps=60]
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from xroute_env_amd.envs.vector_env import XRouteVectorEnv
from xroute_env_amd.lefdef import load_region_pack

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 60
pack = load_region_pack(os.path.join(ROOT, "tests", "golden", "ispd18_test1_regions.npz"))


def rollout(policy):
    env = XRouteVectorEnv(pack, n_envs=B, device="cuda:0", with_observation=False)
    env.reset()
    ret = torch.zeros(B, dtype=torch.float64, device=env.device)       # return of the episode every slot is playing
    total, episodes = 0.0, 0
    for t in range(STEPS):
        actions = env.greedy_actions() if policy == "greedy" else env.random_actions(1234 + t)
        _, reward, done, _ = env.step(actions)                         # (a slot that was done re-initialises: reward -0.0)
        ret += reward
        fin = done.bool()
        total += float(ret[fin].sum())
        episodes += int(fin.sum())
        ret[fin] = 0.0
    return -total / max(episodes, 1), episodes


for policy in ("random", "greedy"):
    cost, episodes = rollout(policy)
    print(f"{policy:6s} ordering: {episodes} episodes of {B} slots x {STEPS} steps, mean episode cost {cost:.1f}")
