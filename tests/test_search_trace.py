"""What the search entry points do on the host on valid calls, pinned as text.

tests/hostsan/search_trace.cpp drives lookahead, rollouts, weighted rollouts, peek, the three tree searches, the evaluated tree search
and branch through the public C ABI against the host-memory HIP stand-in of that directory, with search launchers that report their
arguments (stub_launch_search.cpp): pool bring-up, the shadow view, the carvings, the kept pool's half flip, table reuse, the bank
flips, the eval session's call order, and every allocation of every entry point refused in turn.  It prints one line per launch (every
scalar, every pointer as allocation serial + offset), per hipMalloc, per asynchronous fill or copy, and per call its return code and
the live allocations.  search_trace.expected was recorded while every entry point still wrote its prologue out and the line kernels had
three positional launchers; the shared prologue and the one line launcher are checked against it byte for byte.  The program is built
with ASan + UBSan and runs as a program of its own: a sanitizer report fails it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSAN = os.path.join(ROOT, "tests", "hostsan")
# the loader's experiment switches change the router variant the launches carry: the trace is recorded without them
SWITCHES = ("XR_WINDOW_MARGIN", "XR_NO_MEASURED_ORDER", "XR_HEAVY_CLASS", "XR_HEAVY_MULT", "XR_NO_GUIDE_MASK", "XR_QUEUE_SKIP_SHIFT")


def test_search_calls_match_the_recorded_trace():
    r = subprocess.run(["make", "-C", HOSTSAN, "search_trace"], capture_output=True, text=True)
    assert r.returncode == 0, "build of the trace program failed: " + r.stderr[-1500:]
    assert "warning" not in r.stderr, r.stderr[-1500:]
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([os.path.join(HOSTSAN, "search_trace")], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and out.stdout.endswith("SEARCH_TRACE_OK\n"), (out.stdout[-800:], out.stderr[-3000:])
    assert out.stderr == "", out.stderr[-3000:]
    with open(os.path.join(HOSTSAN, "search_trace.expected")) as f:
        want = f.read()
    if out.stdout != want:
        got_l, want_l = out.stdout.splitlines(), want.splitlines()
        first = next((i for i, (a, b) in enumerate(zip(got_l, want_l)) if a != b), min(len(got_l), len(want_l)))
        call = next((l for l in reversed(want_l[:first + 1]) if not l.startswith(" ")), "?")
        raise AssertionError(f"search trace differs from search_trace.expected at line {first + 1} ({call}):\n"
                             f"  expected: {want_l[first] if first < len(want_l) else '<end>'}\n  got:      {got_l[first] if first < len(got_l) else '<end>'}")
