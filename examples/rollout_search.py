#!/usr/bin/env python3
"""Best-of-R net ordering by rollouts — the classic Monte-Carlo baseline between the random and the learned ordering: at every step each
env plays the rest of its episode R times under the random policy, on the device and without stepping (`XRouteVectorEnv.rollout_actions`:
the first net of the rollout with the highest return), and routes that net.  Beside it the built-in random ordering and the greedy one
(`greedy_actions`: the cheapest next route, one ply), on the regions of ispd18_test1.  Prints the mean episode cost (violations x 500 +
vias x 4 + wirelength x 0.5, the trainers' reward negated) of the three policies over the same regions.

    python examples/rollout_search.py [slots=1024] [steps=60] [R=8]
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from xroute_env_amd.envs.vector_env import XRouteVectorEnv
from xroute_env_amd.lefdef import load_region_pack

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 60
R = int(sys.argv[3]) if len(sys.argv) > 3 else 8
pack = load_region_pack(os.path.join(ROOT, "tests", "golden", "ispd18_test1_regions.npz"))


def play(policy):
    env = XRouteVectorEnv(pack, n_envs=B, device="cuda:0", with_observation=False)
    env.reset()
    ret = torch.zeros(B, dtype=torch.float64, device=env.device)       # return of the episode every slot is playing
    total, episodes = 0.0, 0
    for t in range(STEPS):
        if policy == "greedy":
            actions = env.greedy_actions()
        elif policy == "random":
            actions = env.random_actions(1234 + t)
        else:
            actions = env.rollout_actions(R, 1234 + t)
        _, reward, done, _ = env.step(actions)                         # (a slot that was done re-initialises: reward -0.0)
        ret += reward
        fin = done.bool()
        total += float(ret[fin].sum())
        episodes += int(fin.sum())
        ret[fin] = 0.0
    return -total / max(episodes, 1), episodes


for policy in ("random", "greedy", f"best of {R}"):
    cost, episodes = play(policy)
    print(f"{policy:10s} ordering: {episodes} episodes of {B} slots x {STEPS} steps, mean episode cost {cost:.1f}")
