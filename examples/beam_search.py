#!/usr/bin/env python3
"""Beam search over net orderings (`xroute_env_amd.envs.beam.beam_search`: lookahead -> select -> branch -> step, W lines of play per
region kept on the device) beside the other ordering baselines, on the regions of ispd18_test1: the built-in random ordering, the greedy
one (`greedy_actions`: the cheapest next route, one ply), best of 8 random rollouts (`rollout_actions`), and beams of width 4 and 8.
Every policy plays every region once from its reset; prints the mean episode cost (violations x 500 + vias x 4 + wirelength x 0.5, the
trainers' reward negated).  Beam search is not monotone in its width: a wider beam usually, not always, ends cheaper.

    python examples/beam_search.py [regions=256]
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from xroute_env_amd.envs.beam import beam_search
from xroute_env_amd.envs.vector_env import XRouteVectorEnv
from xroute_env_amd.lefdef import load_region_pack

R = int(sys.argv[1]) if len(sys.argv) > 1 else 256
pack = load_region_pack(os.path.join(ROOT, "tests", "golden", "ispd18_test1_regions.npz"))[:R]
R = len(pack)


def play(policy):
    """One episode of every region (slot r plays region r; a slot's first `done` ends what is counted for it)."""
    env = XRouteVectorEnv(pack, n_envs=R, device="cuda:0", with_observation=False)
    env.batch.assign(list(range(R)))
    env.batch.reset()
    ret = torch.zeros(R, dtype=torch.float64, device=env.device)
    live = torch.ones(R, dtype=torch.bool, device=env.device)
    for t in range(env.kmax + 1):
        if policy == "greedy":
            actions = env.greedy_actions()
        elif policy == "random":
            actions = env.random_actions(1234 + t)
        else:
            actions = env.rollout_actions(8, 1234 + t)
        _, reward, done, _ = env.step(actions)
        ret += torch.where(live, reward, torch.zeros_like(reward))
        live &= ~done.bool()
        if not bool(live.any()):
            break
    return -float(ret.mean())


for policy in ("random", "greedy", "best of 8"):
    print(f"{policy:12s} ordering: mean episode cost {play(policy):.1f} over {R} regions")
for W in (4, 8):
    res = beam_search(pack, W, device="cuda:0")
    cost = -sum(beams[0]["ret"] for beams in res) / R
    print(f"{'beam W = %d' % W:12s} ordering: mean episode cost {cost:.1f} over {R} regions")
