#!/usr/bin/env python3
"""Tree reuse on the regions of ispd18_test1: the tree search of examples/tree_search.py played with a fresh tree at every ply and with
the tree kept ("XR-Tree v1, kept": after the env has stepped net a, the search continues from the root's child of a), at the same
simulations per ply, under the random simulations and under the lookahead weights; and the kept search once more at half the waves from
ply 2 on, which is what the carried visits might buy.  Prints the mean episode cost (violations x 500 + vias x 4 + wirelength x 0.5, the
trainers' reward negated), the nets the searches routed, and what the kept trees carried per ply.  Whether reuse pays on these regions is
not promised: the example prints what it gets.

    python examples/tree_reuse.py [regions=256] [waves=4] [lanes=4] [--temperature 0.25]
"""
import argparse
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from xroute_env_amd.envs.tree import tree_episodes
from xroute_env_amd.envs.weighted import lookahead_weights
from xroute_env_amd.lefdef import load_region_pack

ap = argparse.ArgumentParser()
ap.add_argument("regions", nargs="?", type=int, default=256)
ap.add_argument("waves", nargs="?", type=int, default=4)
ap.add_argument("lanes", nargs="?", type=int, default=4)
ap.add_argument("--temperature", type=float, default=0.25, help="of the lookahead weights, relative to the spread of an env's rewards")
a = ap.parse_args()
pack = load_region_pack(os.path.join(ROOT, "tests", "golden", "ispd18_test1_regions.npz"))[:a.regions]
R = len(pack)
half = max(1, a.waves // 2)

for sims, sim in (("random sims", None), ("weighted sims", lambda batch: lookahead_weights(batch, a.temperature))):
    for name, kw in (("fresh every ply", dict()), ("kept", dict(reuse=True)), ("kept, %d waves after ply 1" % half, dict(reuse=True, waves_after=half))):
        stats = {}
        out = tree_episodes(pack, a.waves, a.lanes, seed=1234, device="cuda:0", stats=stats, sim_weights=sim, **kw)
        line = (f"tree {a.waves} x {a.lanes}, {sims:13s} {name:26s}: mean episode cost {-sum(o['ret'] for o in out) / R:.1f} over {R} regions "
                f"({stats['routed_nets']} nets routed by the searches)")
        if "carried_visits" in stats:
            line += (f"; carried per ply and region {stats['carried_visits'] / max(stats['plies'], 1):.2f} visits, "
                     f"{stats['carried_nodes'] / max(stats['plies'], 1):.1f} nodes")
        print(line, flush=True)
