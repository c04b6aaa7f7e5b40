"""Env front-ends over the batched MI355X hot path.

`facade`      single-env gym-style classes carrying the names the reference registers / reserves
              (reference xroute_env/__init__.py:3-6, xroute_env/envs/*.py are empty stubs)
`vector_env`  the batched form: B regions per call, everything stays on the device
`beam`        beam search over net orderings: lookahead -> select -> branch -> step (`from xroute_env_amd.envs.beam import beam_search`)
`tree`        tree search episodes: one device-side MCTS (RegionBatch.tree_search) per ply, the most visited net stepped
              (`from xroute_env_amd.envs.tree import tree_episodes`)
`weighted`    weights for the weighted net sampling (XR-Pick v1: RegionBatch.weighted_actions, rollout(policy="weighted"),
              tree_search(sim_weights=...)) and a cross-entropy search over orderings on top of it
              (`from xroute_env_amd.envs.weighted import cem_search, lookahead_weights`)
`peek`        successor states and their values on RegionBatch.peek: every candidate net's successor as head rows, a critic value per
              successor, the value-greedy action and the value prior of a tree search
              (`from xroute_env_amd.envs.peek import successor_values, value_actions, value_prior`)
"""
from .facade import OrderingEvaluationEnv, OrderingTrainingEnv, StaticRegionEnv, XRouteEnv
from .vector_env import XRouteVectorEnv

__all__ = ["XRouteEnv", "OrderingTrainingEnv", "OrderingEvaluationEnv", "StaticRegionEnv", "XRouteVectorEnv"]
