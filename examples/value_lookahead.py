#!/usr/bin/env python3
"""A critic asked about states the envs are not in, on the regions of ispd18_test1: peek (RegionBatch.peek) gives the packed state after
every candidate net of every env, expand_state the head rows, the obstacle tower and the critic a value per successor
(`envs.peek.successor_values`).  Four orderings are compared —

  random         a random legal net per ply;
  greedy         the net of the highest one-step reward (lookahead);
  value-greedy   the net of the highest reward + critic value of the successor state (`envs.peek.value_actions`);
  tree, value prior  the tree search whose prior is the softmax of reward + value (`envs.peek.value_prior`), the most visited net stepped.

THE CRITIC IS UNTRAINED: a seeded, randomly initialised ActorCritic.  Its values carry no information about routing cost, so the
value-greedy and value-prior rows say nothing about what a trained critic would do — this example shows the plumbing (three enqueue-only
calls per ply: peek, expand, tower + critic), not a result.

    python examples/value_lookahead.py [regions=256] [waves=4] [lanes=4] [--temperature 0.25]
"""
import argparse
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from xroute_env_amd.agents import ActorCritic, FusedObstacleTower
from xroute_env_amd.envs import peek as pk
from xroute_env_amd.envs.vector_env import XRouteVectorEnv
from xroute_env_amd.lefdef import load_region_pack

ap = argparse.ArgumentParser()
ap.add_argument("regions", nargs="?", type=int, default=256)
ap.add_argument("waves", nargs="?", type=int, default=4)
ap.add_argument("lanes", nargs="?", type=int, default=4)
ap.add_argument("--temperature", type=float, default=0.25, help="of the value prior, relative to the spread of an env's scores")
a = ap.parse_args()
pack = load_region_pack(os.path.join(ROOT, "tests", "golden", "ispd18_test1_regions.npz"))[:a.regions]
R = len(pack)
DEV = "cuda:0"
torch.manual_seed(7)
model = ActorCritic(device=DEV).to(DEV).eval()
shapes = sorted({tuple(int(v) for v in r.dims) for r in pack})
towers = {s: FusedObstacleTower(model.representation_network, (s[2], s[1], s[0]), DEV) for s in shapes}
print(f"critic: ActorCritic with torch.manual_seed(7), UNTRAINED — the value rows below show the plumbing, not a trained critic's quality; "
      f"{sum(t.supported for t in towers.values())} of {len(shapes)} grid shapes take the fused obstacle tower")


def play(policy):
    """One episode of every region (slot r plays region r; a slot's first `done` ends what is counted for it)."""
    env = XRouteVectorEnv(pack, n_envs=R, device=DEV, with_observation=False)
    env.batch.assign(list(range(R)))
    env.batch.reset()
    groups = pk.shape_groups(env.batch)          # (the slots keep their regions for the episode: one host round trip, here)
    ret = torch.zeros(R, dtype=torch.float64, device=env.device)
    live = torch.ones(R, dtype=torch.bool, device=env.device)
    for t in range(env.kmax + 1):
        if policy == "greedy":
            actions = env.greedy_actions()
        elif policy == "random":
            actions = env.random_actions(1234 + t)
        elif policy == "value":
            actions = pk.value_actions(model, env.batch, towers, groups=groups)
        else:
            values, rewards = pk.successor_values(model, env.batch, towers, return_rewards=True, groups=groups)
            prior, _ = pk.value_prior(values, rewards, a.temperature)
            actions = env.tree_actions(a.waves, a.lanes, 1234 + t, prior=prior)
        _, reward, done, _ = env.step(actions)
        ret += torch.where(live, reward, torch.zeros_like(reward))
        live &= ~done.bool()
        if not bool(live.any()):
            break
    return -float(ret.mean())


for policy, name in (("random", "random"), ("greedy", "greedy"), ("value", "value-greedy (untrained)"),
                     ("tree", "tree %d x %d, value prior (untrained)" % (a.waves, a.lanes))):
    print(f"{name:38s} ordering: mean episode cost {play(policy):.1f} over {R} regions")
