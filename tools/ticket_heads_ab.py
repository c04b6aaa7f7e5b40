"""A/B of library builds under bench.py's headline, builds alternating run by run on one machine in one visit:

    python tools/ticket_heads_ab.py --libs parent=libxroute_hip_ab_parent.so this=libxroute_hip.so [more=...] \
        --envs 4096 1024 512 --runs 5 [--dump-compare] --out profiles/step_ticket_heads_ab.json

Every run is `python bench.py --gpus 1 --steps 20 --warmup 3 --envs E` with XR_LIB set (a file name inside xroute_env_amd/).  The first
build is the baseline.  Per batch size and build: median, min, max and spread of env-steps/s; per build against the baseline the bar of
LAB_NOTES §12 — at the headline batch (4096 envs) the gain of the medians must exceed three times the baseline's min-max spread with every run above
the baseline's median, at the smaller ones the median may not fall below the baseline's by more than its spread.  --dump-compare: one
`--dump-outputs` run per build at the first batch size, every .npy compared byte for byte with the baseline's."""
import argparse, filecmp, json, os, statistics, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench(lib, envs, extra=()):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3", "--envs", str(envs), *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, XR_LIB=lib), timeout=600)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    if out.returncode != 0 or not lines:
        sys.exit(f"bench.py failed for {lib} at {envs} envs (exit {out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs="+", required=True, help="name=file, the baseline first")
    ap.add_argument("--envs", nargs="+", type=int, default=[4096, 1024, 512])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--headline-envs", type=int, default=4096, help="the batch size that must show the gain; the others must not lose")
    ap.add_argument("--dump-compare", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    libs = [a.split("=", 1) for a in args.libs]
    base = libs[0][0]
    res = {"what": "bench.py --gpus 1 --steps 20 --warmup 3 --envs E per run, builds alternating run by run, one machine, one visit; "
                   "value = env-steps/s", "builds": dict(libs), "runs": {}, "summary": {}, "bar": {}}
    if args.dump_compare:
        dirs = {}
        with tempfile.TemporaryDirectory() as tmp:
            for name, lib in libs:
                dirs[name] = os.path.join(tmp, name)
                bench(lib, args.envs[0], ("--dump-outputs", dirs[name]))
            files = sorted(os.listdir(dirs[base]))
            res["outputs"] = {}
            for name, _ in libs[1:]:
                _, mismatch, errors = filecmp.cmpfiles(dirs[base], dirs[name], files, shallow=False)
                same = not mismatch and not errors and sorted(os.listdir(dirs[name])) == files
                res["outputs"][name] = f"{len(files)} files byte-equal with {base}" if same else f"DIFFER: {mismatch + errors}"
                print("outputs", name, res["outputs"][name], flush=True)
    for envs in args.envs:
        runs = {name: [] for name, _ in libs}
        for rep in range(args.runs):
            for name, lib in libs:
                d = bench(lib, envs)
                runs[name].append(d["value"])
                print(envs, rep, name, d["value"], flush=True)
        res["runs"][str(envs)] = runs
        summ = {}
        for name, v in runs.items():
            med = statistics.median(v)
            summ[name] = {"runs": len(v), "median_value": med, "min_value": min(v), "max_value": max(v), "spread_value": round(max(v) - min(v), 1),
                          "median_ms_per_step": round(envs / med * 1e3, 4)}
        res["summary"][str(envs)] = summ
        b = summ[base]
        for name, _ in libs[1:]:
            s = summ[name]
            gain = s["median_value"] - b["median_value"]
            if envs == args.headline_envs:
                ok = gain > 3 * b["spread_value"] and min(runs[name]) > b["median_value"]
            else:
                ok = gain >= -b["spread_value"]
            res["bar"].setdefault(name, {})[str(envs)] = {"gain_pct": round(100 * gain / b["median_value"], 3),
                                                          "gain_over_baseline_spread": round(gain / max(b["spread_value"], 1e-9), 2),
                                                          "runs_above_baseline_median": sum(x > b["median_value"] for x in runs[name]), "clears": bool(ok)}
        print(json.dumps({"envs": envs, "summary": summ, "bar": {n: res["bar"][n][str(envs)] for n, _ in libs[1:]}}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
