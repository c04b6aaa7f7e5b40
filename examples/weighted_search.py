#!/usr/bin/env python3
"""Weighted net sampling beside the other ordering baselines, on the regions of ispd18_test1: the table of examples/tree_search.py
(random, greedy, best of R random rollouts, beam search, tree search) with two more rows at an equal number of routed nets per ply —

  CEM            at every ply a cross-entropy search (`envs.weighted.cem_search`: W iterations of P weighted rollouts, the weights
                 refitted to the elite orderings) and the first net of the best ordering it found is stepped: W * P complete lines per
                 env and ply, as best of R = W * P;
  tree, weighted the tree search whose simulations below a selected node follow the env's lookahead weights
                 (`tree_search(sim_weights=lookahead_weights(batch))`) instead of the uniform random policy; one more route per candidate
                 and ply for the lookahead.

Every policy plays every region once from its reset; prints the mean episode cost (violations x 500 + vias x 4 + wirelength x 0.5, the
trainers' reward negated).  Whether either new row beats best of R is not promised: the example prints what it gets.

    python examples/weighted_search.py [regions=256] [waves=4] [lanes=4] [--elite 4] [--temperature 0.25]
"""
import argparse
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from xroute_env_amd.envs.beam import beam_search
from xroute_env_amd.envs.tree import tree_episodes
from xroute_env_amd.envs.vector_env import XRouteVectorEnv
from xroute_env_amd.envs.weighted import cem_search, lookahead_weights
from xroute_env_amd.lefdef import load_region_pack

ap = argparse.ArgumentParser()
ap.add_argument("regions", nargs="?", type=int, default=256)
ap.add_argument("waves", nargs="?", type=int, default=4)
ap.add_argument("lanes", nargs="?", type=int, default=4)
ap.add_argument("--elite", type=int, default=0, help="elite rollouts per CEM iteration (default: lanes / 2, at least 1)")
ap.add_argument("--temperature", type=float, default=0.25, help="of the lookahead weights, relative to the spread of an env's rewards")
a = ap.parse_args()
pack = load_region_pack(os.path.join(ROOT, "tests", "golden", "ispd18_test1_regions.npz"))[:a.regions]
R, S = len(pack), a.waves * a.lanes
elite = a.elite if a.elite > 0 else max(1, a.lanes // 2)


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
        elif policy == "cem":
            order, _, _ = cem_search(env.batch, a.waves, a.lanes, elite, 1234 + t)
            actions = order[:, 0].contiguous()
        else:
            actions = env.rollout_actions(S, 1234 + t)
        _, reward, done, _ = env.step(actions)
        ret += torch.where(live, reward, torch.zeros_like(reward))
        live &= ~done.bool()
        if not bool(live.any()):
            break
    return -float(ret.mean())


for policy, name in (("random", "random"), ("greedy", "greedy"), ("best", f"best of {S}"), ("cem", "CEM %d x %d" % (a.waves, a.lanes))):
    print(f"{name:18s} ordering: mean episode cost {play(policy):.1f} over {R} regions")
res = beam_search(pack, S, device="cuda:0")
print(f"{'beam W = %d' % S:18s} ordering: mean episode cost {-sum(beams[0]['ret'] for beams in res) / R:.1f} over {R} regions")
for name, sim in (("tree %d x %d" % (a.waves, a.lanes), None),
                  ("tree, weighted sims", lambda batch: lookahead_weights(batch, a.temperature))):
    stats = {}
    out = tree_episodes(pack, a.waves, a.lanes, seed=1234, device="cuda:0", stats=stats, sim_weights=sim)
    print(f"{name:18s} ordering: mean episode cost {-sum(o['ret'] for o in out) / R:.1f} over {R} regions "
          f"({stats['routed_nets']} nets routed by the searches); best line seen {-sum(o['best_ret'] for o in out) / R:.1f}")
