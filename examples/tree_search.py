#!/usr/bin/env python3
"""Tree search over net orderings (`xroute_env_amd.envs.tree.tree_episodes`: at every ply one device-side MCTS per env,
`RegionBatch.tree_search`, then the most visited net is stepped) beside the other ordering baselines, on the regions of ispd18_test1:
the built-in random ordering, the greedy one (`greedy_actions`), best of R random rollouts (`rollout_actions`) and beam search
(`envs.beam.beam_search`) — at an equal number of routed nets per ply: a tree search of W waves x P lanes routes W * P complete lines
from every env, as best of R = W * P does; a beam of width W * P prices at most that many (beam, net) pairs of one route each.  Every
policy plays every region once from its reset; prints the mean episode cost (violations x 500 + vias x 4 + wirelength x 0.5, the
trainers' reward negated) and, for the tree, also the best complete ordering any simulation saw.

    python examples/tree_search.py [regions=256] [waves=4] [lanes=4] [--prior lookahead] [--temperature 50]

--prior lookahead: the prior of every search is the softmax of the env's lookahead rewards over the temperature (one more route per
candidate and ply); default: the uniform prior.
"""
import argparse
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from xroute_env_amd.envs.beam import beam_search
from xroute_env_amd.envs.tree import lookahead_prior, tree_episodes
from xroute_env_amd.envs.vector_env import XRouteVectorEnv
from xroute_env_amd.lefdef import load_region_pack

ap = argparse.ArgumentParser()
ap.add_argument("regions", nargs="?", type=int, default=256)
ap.add_argument("waves", nargs="?", type=int, default=4)
ap.add_argument("lanes", nargs="?", type=int, default=4)
ap.add_argument("--prior", choices=("uniform", "lookahead"), default="uniform")
ap.add_argument("--temperature", type=float, default=50.0)
a = ap.parse_args()
pack = load_region_pack(os.path.join(ROOT, "tests", "golden", "ispd18_test1_regions.npz"))[:a.regions]
R, S = len(pack), a.waves * a.lanes


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
            actions = env.rollout_actions(S, 1234 + t)
        _, reward, done, _ = env.step(actions)
        ret += torch.where(live, reward, torch.zeros_like(reward))
        live &= ~done.bool()
        if not bool(live.any()):
            break
    return -float(ret.mean())


for policy in ("random", "greedy", f"best of {S}"):
    print(f"{policy:16s} ordering: mean episode cost {play(policy):.1f} over {R} regions")
res = beam_search(pack, S, device="cuda:0")
print(f"{'beam W = %d' % S:16s} ordering: mean episode cost {-sum(beams[0]['ret'] for beams in res) / R:.1f} over {R} regions")
prior = (lambda batch: lookahead_prior(batch, a.temperature)) if a.prior == "lookahead" else None
stats = {}
out = tree_episodes(pack, a.waves, a.lanes, seed=1234, device="cuda:0", prior=prior, stats=stats)
name = "tree %d x %d" % (a.waves, a.lanes)
print(f"{name:16s} ordering: mean episode cost {-sum(o['ret'] for o in out) / R:.1f} over {R} regions ({a.prior} prior, "
      f"{stats['routed_nets']} nets routed by the searches)")
print(f"{'':16s} best line seen: mean episode cost {-sum(o['best_ret'] for o in out) / R:.1f}")
