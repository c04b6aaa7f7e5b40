"""What xr_batch_load_regions decides and uploads, pinned as text.

tests/hostsan/load_trace.cpp drives the loader through the public C ABI against the host-memory HIP stand-in of that directory, for a
list of cases that takes every branch of the loader (every router form, the window form, the sweeps of a large batch, every refusal,
the allocation limit at every size, reloads), and prints return codes, messages, hipMalloc sizes in order, the router variant of the
first launches, XrBatchDev and the region table field by field and a hash of every uploaded table.  load_trace.expected was recorded
while the loader was still one function; the loader's steps are checked against it byte for byte.  The program is built with
ASan + UBSan and runs as a program of its own: a sanitizer report fails it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSAN = os.path.join(ROOT, "tests", "hostsan")
# the loader's experiment switches change what it decides: the trace is recorded without them
SWITCHES = ("XR_WINDOW_MARGIN", "XR_NO_MEASURED_ORDER", "XR_HEAVY_CLASS", "XR_HEAVY_MULT", "XR_NO_GUIDE_MASK", "XR_QUEUE_SKIP_SHIFT")


def test_loader_output_matches_the_recorded_trace():
    r = subprocess.run(["make", "-C", HOSTSAN, "load_trace"], capture_output=True, text=True)
    assert r.returncode == 0, "build of the trace program failed: " + r.stderr[-1500:]
    assert "warning" not in r.stderr, r.stderr[-1500:]
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([os.path.join(HOSTSAN, "load_trace")], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and out.stdout.endswith("LOAD_TRACE_OK\n"), (out.stdout[-800:], out.stderr[-3000:])
    assert out.stderr == "", out.stderr[-3000:]
    with open(os.path.join(HOSTSAN, "load_trace.expected")) as f:
        want = f.read()
    if out.stdout != want:
        got_l, want_l = out.stdout.splitlines(), want.splitlines()
        first = next((i for i, (a, b) in enumerate(zip(got_l, want_l)) if a != b), min(len(got_l), len(want_l)))
        case = next((l for l in reversed(want_l[:first + 1]) if l.startswith("case ")), "?")
        raise AssertionError(f"loader trace differs from load_trace.expected at line {first + 1} ({case}):\n"
                             f"  expected: {want_l[first] if first < len(want_l) else '<end>'}\n  got:      {got_l[first] if first < len(got_l) else '<end>'}")
