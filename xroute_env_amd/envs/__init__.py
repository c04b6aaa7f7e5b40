"""Env front-ends over the batched MI355X hot path.

`facade`      single-env gym-style classes carrying the names the reference registers / reserves
              (reference xroute_env/__init__.py:3-6, xroute_env/envs/*.py are empty stubs)
`vector_env`  the batched form: B regions per call, everything stays on the device
`beam`        beam search over net orderings: lookahead -> select -> branch -> step (`from xroute_env_amd.envs.beam import beam_search`)
`tree`        tree search episodes: one device-side MCTS (RegionBatch.tree_search) per ply, the most visited net stepped
              (`from xroute_env_amd.envs.tree import tree_episodes`)
"""
from .facade import OrderingEvaluationEnv, OrderingTrainingEnv, StaticRegionEnv, XRouteEnv
from .vector_env import XRouteVectorEnv

__all__ = ["XRouteEnv", "OrderingTrainingEnv", "OrderingEvaluationEnv", "StaticRegionEnv", "XRouteVectorEnv"]
