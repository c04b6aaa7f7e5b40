"""XR-Pick v1 (include/xroute_hip.h, "---- weighted net sampling") in Python integers: splitmix64, the clamp, the uniform fallback.  The
twin of xr_batch_weighted_actions for the tests: it runs without a GPU on hand-made rows (tests/test_weighted_host.py) and on the fetched
`legal` and `env_steps` of a batch beside the device pick (tests/test_gpu_weighted.py)."""
M64 = 2 ** 64 - 1
WEIGHT_MAX = 1 << 24


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def pick_hash(seed, env, env_steps):
    """r of XR-Pick v1: the bits xr_batch_random_actions uses too."""
    return splitmix64((seed & M64) ^ splitmix64((env * 0x100000001B3 + env_steps) & M64))


def effective(w):
    """q(n): 0 for w <= 0, else min(w, XR_WEIGHT_MAX)."""
    w = int(w)
    return 0 if w <= 0 else min(w, WEIGHT_MAX)


def pick_from_r(legal, weights, r):
    """The pick for the hash value r.  legal: the legal nets (1-based, any order); weights: a sequence with net n at n - 1 (a net beyond
    its end counts 0)."""
    nets = sorted(int(n) for n in legal)
    if not nets:
        return 0
    q = [effective(weights[n - 1]) if n - 1 < len(weights) else 0 for n in nets]
    S = sum(q)
    if S == 0:
        return nets[r % len(nets)]
    t = r % S
    run = 0
    for n, v in zip(nets, q):
        run += v
        if run > t:
            return n
    raise AssertionError("t < S: not reached")


def pick(legal, env_steps, env, seed, weights):
    return pick_from_r(legal, weights, pick_hash(seed, env, int(env_steps)))


def legal_nets(words):
    """The 1-based nets of a row of uint64 legal words (any integer type)."""
    out = []
    for c, m in enumerate(words):
        m = int(m) & M64
        while m:
            low = m & -m
            out.append(c * 64 + low.bit_length())
            m ^= low
    return out
