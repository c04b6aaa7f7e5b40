#!/usr/bin/env python3
"""Independent stepping of env groups: the worker model of the reference's A3C / MCTS trainers (workers that never wait for each other)
on one MI355X.  G env groups of one XRouteVectorEnv are driven by the built-in random policy; each group steps again as soon as its last
step has finished (ready_groups), without waiting for the others.  Reports env-steps/s beside the lock-step loop over the same slots, and
checks at the end that every env's hash chain equals a lock-step twin's at the same number of steps.

    python examples/async_rollout.py [--envs 1024] [--groups 4] [--seconds 3]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from xroute_env_amd.envs import XRouteVectorEnv  # noqa: E402
from xroute_env_amd.regions import config_regions  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--seed", type=int, default=11)
    a = ap.parse_args()
    regions = config_regions(4, 64)
    env = XRouteVectorEnv(regions, n_envs=a.envs, groups=a.groups)
    twin = XRouteVectorEnv(regions, n_envs=a.envs)
    env.reset()
    twin.reset()

    # lock-step loop (the twin): every slot steps together
    torch.cuda.synchronize()
    t0, n_lock = time.perf_counter(), 0
    while time.perf_counter() - t0 < a.seconds:
        twin.step(twin.random_actions(a.seed))
        n_lock += 1
    torch.cuda.synchronize()
    lock_rate = n_lock * a.envs / (time.perf_counter() - t0)

    # groups: a group steps again as soon as its own last step has finished
    counts = [0] * env.n_groups
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < a.seconds:
        for g in env.ready_groups():
            s = env.group_streams[g]
            with torch.cuda.stream(s):
                acts = env.batch.random_actions_group(g, a.seed, stream=s)
            env.step_async(acts, group=g)
            counts[g] += 1
    env.step_wait()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    sizes = [hi - lo for lo, hi in (env.batch.group_bounds(g) for g in range(env.n_groups))]
    group_rate = sum(c * s for c, s in zip(counts, sizes)) / dt
    print(f"lock-step: {lock_rate / 1e6:.3f} M env-steps/s ({n_lock} steps of {a.envs} slots)")
    print(f"{env.n_groups} groups: {group_rate / 1e6:.3f} M env-steps/s (steps per group: {counts})")

    # hash chains: a fresh lock-step twin, its slices captured after as many steps as each group took
    check = XRouteVectorEnv(regions, n_envs=a.envs)
    check.reset()
    want = {}
    for t in range(1, max(counts) + 1):
        check.step(check.random_actions(a.seed))
        for g, c in enumerate(counts):
            if c == t:
                lo, hi = env.batch.group_bounds(g)
                want[g] = check.batch.fetch("hash")[lo:hi].clone()
    got = env.batch.fetch("hash")
    ok = all(torch.equal(got[slice(*env.batch.group_bounds(g))], want[g]) for g in range(env.n_groups) if counts[g])
    print("hash chains equal the lock-step twin's:", ok)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
