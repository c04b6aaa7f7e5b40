#!/usr/bin/env python3
"""A/B of the uint8 observation (xr_batch_step_observe_u8) against fp32: the full step (random net-order action + route + observation of
every env) in four forms — fp32 full write, fp32 in place, u8 full write, u8 in place — alternated in one process on twin batches.

Points: i512 / i1024 / i4096   ispd18_test1-sized regions (24x40x9, config 4), that many slots
        pack256                the 256 regions extracted from ispd18_test1 (tests/golden/ispd18_test1_regions.npz), 256 slots

One JSON line per (point, form): ms per step, env-steps/s, algorithmic observation bytes per step (4·N·(2+7K) fp32, N·(2+7K) u8, K =
the slots' nets left after the step) and their fraction of 8 TB/s, and whether u8 rows equal the fp32 rows cast to bytes in a sample of
envs.  Without --point every point runs in a child process under its own `timeout`, stopping at the first failure.

    python tools/obs_u8_ab.py [--steps 20] [--warmup 5] [--reps 3] [--point i4096] [--json profiles/obs_u8_ab.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POINTS = {"i512": 512, "i1024": 1024, "i4096": 4096, "pack256": 256}
FORMS = ("fp32_full", "fp32_inplace", "u8_full", "u8_inplace")
SEED = 91
HBM_PEAK = 8.0e12


def run_point(name, steps, warmup, reps):
    import numpy as np
    import torch
    from xroute_env_amd.batch import RegionBatch
    from xroute_env_amd.regions import config_regions
    n = POINTS[name]
    if name == "pack256":
        from xroute_env_amd.lefdef import load_region_pack
        regions = load_region_pack(os.path.join(ROOT, "tests", "golden", "ispd18_test1_regions.npz"))
    else:
        regions = config_regions(4, 256)
    dev = "cuda:0"
    bat = {f: RegionBatch(regions, n_envs=n, device=dev, auto_reset=True) for f in FORMS}
    obs = {}
    for f, b in bat.items():
        b.reset(rotate=True)
        obs[f] = b.alloc_observation(dtype=torch.uint8 if f.startswith("u8") else torch.float32).zero_()
        b.observation(obs[f])
    act = torch.empty(n, dtype=torch.int32, device=dev)
    nodes = torch.tensor([r.n_nodes for r in regions], dtype=torch.float64, device=dev)

    def run(f, k):
        b = bat[f]
        for _ in range(k):
            b.random_actions(SEED, act)
            b.step(act, obs[f], inplace=f.endswith("inplace"))

    times = {f: [] for f in FORMS}
    bytes_per_step = {f: [] for f in FORMS}
    for _ in range(reps):
        for f in FORMS:
            run(f, warmup)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(f, steps)
            e1.record()
            e1.synchronize()
            times[f].append(e0.elapsed_time(e1) / steps)
            b = bat[f]
            vals = (2 + 7 * b.fetch("nlegal").double()) * nodes[b.fetch("region").long()]
            bytes_per_step[f].append(float(vals.sum()) * (1 if f.startswith("u8") else 4))
    # every batch took the same number of steps with the same policy: u8 rows == fp32 rows cast, sampled envs
    torch.cuda.synchronize()
    ref = bat["fp32_full"]
    same_state = all(torch.equal(ref.fetch("hash"), bat[f].fetch("hash")) for f in FORMS)
    reg = ref.fetch("region").cpu().numpy()
    nl = ref.fetch("nlegal").cpu().numpy()
    rows_ok = True
    for e in range(0, n, max(1, n // 64)):
        m = (2 + 7 * int(nl[e])) * regions[int(reg[e])].n_nodes
        want = obs["fp32_full"][e, :m].to(torch.uint8)
        rows_ok &= bool(torch.equal(obs["u8_full"][e, :m], want) and torch.equal(obs["u8_inplace"][e, :m], want))
    out = []
    for f in FORMS:
        ms = float(np.median(times[f]))
        by = float(np.mean(bytes_per_step[f]))
        rec = {"point": name, "envs": n, "form": f, "ms_per_step": round(ms, 4), "env_steps_per_s": round(n / ms * 1e3),
               "obs_bytes_per_step": int(by), "obs_bw_frac_of_8TBps": round(by / (ms * 1e-3) / HBM_PEAK, 4),
               "reps_ms": [round(t, 4) for t in times[f]], "same_state": same_state, "u8_rows_equal_fp32_cast": rows_ok}
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return same_state and rows_ok, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--point", choices=list(POINTS))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per point (child processes)")
    ap.add_argument("--json", help="also write every line to this file (one JSON document)")
    a = ap.parse_args()
    if a.point:
        ok, _ = run_point(a.point, a.steps, a.warmup, a.reps)
        sys.exit(0 if ok else 1)
    lines = []
    for p in POINTS:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--point", p, "--steps", str(a.steps),
               "--warmup", str(a.warmup), "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        lines += [json.loads(s) for s in r.stdout.splitlines() if s.startswith("{")]
        if r.returncode != 0:
            print(json.dumps({"point": p, "error": f"exit status {r.returncode}", "stderr": r.stderr[-2000:]}), flush=True)
            break
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"tool": "tools/obs_u8_ab.py", "steps": a.steps, "warmup": a.warmup, "reps": a.reps, "results": lines}, fh, indent=1)
    sys.exit(0 if all(l.get("same_state") and l.get("u8_rows_equal_fp32_cast") for l in lines) and len(lines) == 4 * len(POINTS) else 1)


if __name__ == "__main__":
    main()
