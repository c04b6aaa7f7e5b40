"""Host side of the tower shape sweep (tests/test_gpu_tower_shapes.py): the two acceptance predicates of the fused towers against the launchers' own
conditions, and proof that the sweep's inputs can see a border mistake.  CPU only."""
import copy

import pytest
import torch

from tests import tower_shapes as ts
from xroute_env_amd import agents


# ---- the launchers' acceptance conditions, restated from csrc/xr_agent.hip (quoted: the line each step comes from) ----
def _launcher_common(shape):
    D, H, W = shape
    strd = lambda s, t: ((s - t + t - 1) // t if s > t else 0) + 1                              # xr_agent.hip `strd`: ceil(max(0, s - t) / t) + 1
    sd, sh, sw = strd(D, 3), strd(H, 64), strd(W, 64)
    if D + 2 < 5 or H + 2 < 5 or W + 2 < 5:                                                     # "if (D + 2 < 5 || H + 2 < 5 || W + 2 < 5) return XR_ERR_RANGE"
        return None
    od, oh, ow = (D + 2 - 5) // sd + 1, (H + 2 - 5) // sh + 1, (W + 2 - 5) // sw + 1
    if od > 3 or oh + 3 > 64 or ow + 3 > 64:                                                    # "if (g.od > 3 || g.oh + 3 > 64 || g.ow + 3 > 64 ..."
        return None
    return sd, sh, sw, od, oh, ow, 7 * od * oh * ow, 21 * (oh + 3) * (ow + 3)


def launcher_takes_obstacle(shape, threads: int) -> bool:
    """`xr_agent_obstacle_tower`'s conditions on (D, H, W) (the head's stride aside) for a workgroup of `threads`: 768 in matrix mode 1, 1024 in mode 0"""
    D, H, W = shape
    c = _launcher_common(shape)
    if c is None:
        return False
    sd, sh, sw, od, oh, ow, nB, nC1 = c
    Np = (D + 2) * (H + 2) * ((W + 2) | 1)                                                      # "const int64_t Np = ..."
    y_in_b = Np <= nB                                                                           # "g.y_in_b = Np <= nB"
    c1_alloc = max(nC1, Np if y_in_b else 2 * Np)                                               # "const int64_t c1_alloc = ..."
    if nB < 1024 * 3:                                                                           # "if (nB < 1024 * 3 || head_stride < N) return XR_ERR_RANGE"
        return False
    lds = (nB + c1_alloc + 8 + (threads // 64) * (ow + 2 + 2) * 3) * 4                          # "const size_t lds = ... (threads / 64) * (g.cols + 2) * 3 ..."
    return lds <= 160 * 1024                                                                    # "if (lds > 160 * 1024) return XR_ERR_RANGE"


def launcher_takes_net(shape) -> bool:
    """`xr_launch_net_tower`'s conditions on (D, H, W)"""
    D, H, W = shape
    c = _launcher_common(shape)
    if c is None or D * H * W >= 65536:                                                         # "... || (int64_t)D * H * W >= 65536"
        return False
    sd, sh, sw, od, oh, ow, nB, nC1 = c
    fixed = 6 * D * H + 256 + 8 + 112 + 952                                                     # "const int64_t fixed = ..."
    if nB < 1024 * 3 or nC1 < fixed + 1024 or W > 32 or D > 32 or H > 64 or sh != 1 or sw != 1:  # "if (nB < 1024 * 3 || nC1 < fixed + 1024 || W > 32 ..."
        return False
    return (nB + nC1 + 8 + 16 * (ow + 2 + 2) * 3) * 4 <= 160 * 1024                             # "const size_t lds = ...; if (lds > 160 * 1024)"


def _around(values, lo=1):
    return sorted({v + d for v in values for d in (-1, 0, 1) if v + d >= lo})


def test_obstacle_tower_predicate_against_the_launcher():
    """`FusedObstacleTower.accepts` (what `supported` starts as) against `xr_agent_obstacle_tower`'s conditions, on a grid of shapes around every limit:
    the smallest grid (3), the depth strides' steps, H / W = 64 (strides 2 and 3 begin behind it) .. 130, the margin (oh + 3, ow + 3 <= 64), the smallest
    b (7 od oh ow >= 3072), y in b's space or behind x, and the 160 KB of LDS — plus every shape of the sweep.
    With 1024 threads (matrix mode 0: 16 waves) the two agree everywhere.  With 768 threads (matrix mode 1, the default: 12 waves) Python is the STRICTER side
    by design: its `tail` counts 16 waves' column sums whatever the mode, so that `supported` does not depend on an environment variable of the library —
    the launcher takes everything Python accepts, and the only shapes it takes beyond are within 4 waves' sums (4 x 3 (ow + 4) floats) of the LDS limit."""
    Ds = _around([3, 4, 6, 7, 9, 10, 12, 14, 32, 39])
    HWs = _around([3, 10, 13, 17, 22, 25, 32, 34, 58, 63, 64, 66, 80, 128, 129])
    seen = {"both": 0, "neither": 0, "launcher768_only": 0}
    shapes = {(D, H, W) for D in Ds for H in HWs for W in HWs} | set(ts.OB_SHAPES)
    # ... and a band around the LDS limit itself: every (H, W) of a few depths whose footprint is within 1 KB of it
    for D in (4, 9, 12, 14, 32):
        for H in range(3, 70):
            for W in range(3, 70):
                g = ts.geometry((D, H, W))
                n_p = (D + 2) * (H + 2) * ((W + 2) | 1)
                foot = 4 * (g["nB"] + max(g["nC1"], n_p if n_p <= g["nB"] else 2 * n_p) + 8 + 48 * (g["ow"] + 4))
                if abs(foot - 160 * 1024) <= 1024:
                    shapes.add((D, H, W))
    for s in sorted(shapes):
        py, l16, l12 = agents.FusedObstacleTower.accepts(s), launcher_takes_obstacle(s, 1024), launcher_takes_obstacle(s, 768)
        assert py == l16, (s, py, l16)
        assert l12 or not py, (s, "Python accepts what the launcher refuses with 768 threads")
        if l12 and not py:
            g = ts.geometry(s)
            n_p = (s[0] + 2) * (s[1] + 2) * ((s[2] + 2) | 1)
            foot12 = 4 * (g["nB"] + max(g["nC1"], n_p if n_p <= g["nB"] else 2 * n_p) + 8 + 36 * (g["ow"] + 4))
            assert 160 * 1024 - 4 * 12 * (g["ow"] + 4) < foot12 <= 160 * 1024, (s, foot12)
        seen["both" if py else "launcher768_only" if l12 else "neither"] += 1
    assert min(seen.values()) > 0, seen                       # the grid reaches both sides of the limits, and the one-sided band
    assert all(agents.FusedObstacleTower.accepts(s) for s in ts.OB_SHAPES)
    # (14, 32, 22) sits ON the limit: b 12 600 floats, x and y behind one another 2 x 13 600 (y does not fit b's space), 8 zero words, 16 waves' sums
    assert ts.geometry((14, 32, 22))["nB"] == 12600 and 16 * 34 * 25 == 13600 and 4 * (12600 + 2 * 13600 + 8 + 16 * 24 * 3) == 160 * 1024
    assert agents.FusedObstacleTower.accepts((14, 32, 22)) and not agents.FusedObstacleTower.accepts((14, 32, 23))


def test_net_tower_predicate_against_the_launcher():
    """`FusedNetTower.accepts` against `xr_launch_net_tower`'s conditions: the same on every shape (both count 16 waves: the net variant always runs 1024
    threads) — around W = 32, D = 32, H = 63 / 64 (the packed coordinates and the margin), the smallest b, the front end's fixed part + 1024 words against
    the first activation's space, and the LDS limit."""
    Ds = _around([3, 5, 6, 9, 12, 30, 32])
    Hs = _around([3, 7, 12, 15, 17, 22, 34, 52, 58, 63, 64])
    Ws = _around([3, 5, 17, 19, 22, 25, 32])
    n_yes = 0
    for s in sorted({(D, H, W) for D in Ds for H in Hs for W in Ws} | set(ts.NET_SHAPES) | {(D, H, W) for D in (12, 32) for H in range(3, 66) for W in (5, 17, 32)}):
        py, la = agents.FusedNetTower.accepts(s), launcher_takes_net(s)
        assert py == la, (s, py, la)
        n_yes += py
    assert n_yes > 100
    assert all(agents.FusedNetTower.accepts(s) for s in ts.NET_SHAPES)
    for s in ((3, 17, 33), (33, 12, 17), (3, 64, 10), (3, 70, 24)):         # one past W = 32, D = 32, H = 63; sh = 2
        assert not agents.FusedNetTower.accepts(s), s


def test_the_constructors_use_the_predicates():
    """`supported` is `accepts(dims)` — the towers take no other decision about a shape (construction on the CPU: nothing is launched)"""
    rep = ts.make_rep()
    for s, want in (((3, 22, 24), True), ((12, 70, 70), False), ((2, 2, 2), False)):
        assert agents.FusedObstacleTower(rep, s, "cpu").supported == agents.FusedObstacleTower.accepts(s) == want
    for s, want in (((3, 17, 32), True), ((3, 17, 33), False)):
        assert agents.FusedNetTower(rep, s, "cpu").supported == agents.FusedNetTower.accepts(s) == want


def test_the_fp64_reference_is_the_modules_own_path_in_double():
    """The sweep's reference runs the plain 3-D convolutions on the whole padded standard grid; the module's shortcuts (cropped padding, folded depth) give
    the same numbers in fp64 (1e-12), and its fp32 path is within 5e-6 of them: the 2e-4 bound is left whole for the kernels."""
    for s in ((7, 34, 25), (3, 129, 13)):
        D, H, W = s
        g = ts.ob_grids(s).reshape(5, 1, D, H, W)
        with torch.no_grad():
            fold = agents.normalize(copy.deepcopy(ts.make_rep()).double().encode_obstacles(g.double()))
            f32 = agents.normalize(ts.make_rep().encode_obstacles(g))
        assert float((fold - ts.ob_reference(s)).abs().max()) <= 1e-12
        assert float((f32 - ts.ob_reference(s)).abs().max()) <= 5e-6
    s = (6, 52, 22)
    for wset in ts.WEIGHT_SETS:
        planes = ts.pairs_of(ts.net_regions(s))[2]
        with torch.no_grad():
            fold = agents.normalize(copy.deepcopy(ts.make_rep(wset)).double().encode_nets(planes.double()))
            f32 = agents.normalize(ts.make_rep(wset).encode_nets(planes))
        assert float((fold - ts.net_reference(s, wset)).abs().max()) <= 1e-12
        assert float((f32 - ts.net_reference(s, wset)).abs().max()) <= 2e-5, wset


# The border slices the obstacle reference provably ignores: the aligning convolution's last depth tap reads slice (od - 1) sd + 3, the 1-channel block
# in front of it carries a voxel two slices far, so slice D - 1 counts iff D - 3 <= (od - 1) sd + 3.  sd = 11 at D = 32: taps up to slice 25; sd = 13 at
# D = 39: up to 29.  (H and W: the same with sh / sw — every shape of the sweep reaches its last row and column; the first slices are always read.)
OB_IGNORED = {(32, 19, 21): {"d_hi"}, (39, 12, 17): {"d_hi"}}
BORDERS = ("d_lo", "d_hi", "h_lo", "h_hi", "w_lo", "w_hi")


@pytest.mark.parametrize("shape", ts.OB_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_obstacle_sweep_can_see_a_border_mistake(shape):
    """Blanking any of the six border slices of each random grid of the sweep moves its fp64 vector by at least 10 x the sweep's tolerance (measured: >= 1.4e-2),
    so a kernel that drops or misplaces a border row, column or slice cannot pass — except the slices the reference itself ignores (OB_IGNORED), where the
    vector does not move at all."""
    D, H, W = shape
    g = ts.geometry(shape)
    ref = ts.ob_reference(shape)
    for b, name in enumerate(BORDERS):
        ax, hi = b // 2, b % 2
        n, o, s = shape[ax], (g["od"], g["oh"], g["ow"])[ax], (g["sd"], g["sh"], g["sw"])[ax]
        ignored = bool(hi) and n - 3 > (o - 1) * s + 3
        assert ignored == (name in OB_IGNORED.get(shape, ())), (shape, name)
        blank = ts.ob_grids(shape).reshape(5, D, H, W).clone()
        idx = [slice(None)] * 4
        idx[ax + 1] = n - 1 if hi else 0
        blank[tuple(idx)] = 0.0
        moved = (ts.ob_vectors64(shape, blank.reshape(5, -1)) - ref).abs().amax(dim=1)[2:]         # the three random grids
        if ignored:
            assert float(moved.max()) == 0.0, (shape, name, moved.tolist())
        else:
            assert float(moved.min()) >= 10 * ts.TOL, (shape, name, moved.tolist())


# Corners whose access point the net reference ignores: an access point changes the block's output within two voxels, and at D = 30 (sd = 10) / D = 32
# (sd = 11) the aligning convolution's last depth tap reads slice 23 / 25: the four corners of the last slice
NET_IGNORED = {(30, 7, 32): {4, 5, 6, 7}, (32, 12, 17): {4, 5, 6, 7}}


@pytest.mark.parametrize("weights", ts.WEIGHT_SETS)
@pytest.mark.parametrize("shape", ts.NET_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_net_sweep_can_see_a_corner_access_point(shape, weights):
    """A net of the centre voxel and one corner access point (adjacency planes on, as the corner nets of the sweep's part 3 (a) with the flag): dropping the
    corner moves the fp64 vector by at least 10 x the tolerance (measured: >= 7e-3) or, at the corners of NET_IGNORED, not at all.  (A lone corner WITHOUT the
    flag lights one voxel of one plane and moves the vector by as little as 1.3e-3 with these weights: still 6 x the tolerance, which is why the sweep runs
    both kinds.)"""
    D, H, W = shape
    g = ts.geometry(shape)
    mid = ((D // 2) * H + H // 2) * W + W // 2
    cs = ts.corners(shape)
    v = ts.net_vectors64(weights, torch.stack([ts.host_planes(shape, [mid], [0])] + [ts.host_planes(shape, [c, mid], [1, 0]) for c in cs]))
    moved = (v[1:] - v[0]).abs().amax(dim=1)
    for i in range(8):
        ignored = cs[i] // (H * W) == D - 1 and D - 3 > (g["od"] - 1) * g["sd"] + 3
        assert ignored == (i in NET_IGNORED.get(shape, ())), (shape, i)
        if ignored:
            assert float(moved[i]) == 0.0, (shape, weights, i, float(moved[i]))
        else:
            assert float(moved[i]) >= 10 * ts.TOL, (shape, weights, i, float(moved[i]))


def test_the_sweeps_nets_fit_and_the_boundary_nets_straddle_the_limit():
    """The host prediction of the net tower's list capacity (S1 = access points dilated by one voxel, S2 by two, against the launcher's nB and nC1) says that
    every generated and hand-built net of the sweep fits, and that the grown nets of part 3 (f) straddle the limit they are meant to: S1 binds first at
    (3, 17, 32) on a lattice 3 apart, S2 on one 5 apart; at (12, 34, 25) S2 binds first whatever the lattice (7.5 n2 <= 15 334 against 7.5 n1 <= 15 456, and
    n2 >= n1): no S1 case there."""
    for s in ts.NET_SHAPES:
        nets = [f for r in ts.net_regions(s) for f, _ in ts.region_nets(r)]
        assert all(len(r.nodes) == s[0] * s[1] * s[2] and r.n_nets <= 12 for r in ts.net_regions(s))
        assert len(nets) >= 8 and all(all(ts.net_fits(s, f)[2:]) for f in nets), s
    for s in ts.HAND_SHAPES:
        regions, names = ts.hand_regions(s)
        for r, nm in zip(regions, names):
            nets = ts.region_nets(r)
            assert len(nets) == len(nm) and all(all(ts.net_fits(s, f)[2:]) for f, _ in nets), s
        assert max(len(f) for r in regions for f, _ in ts.region_nets(r)) == 128
        flags = [int(a.max()) for f, a in ts.region_nets(regions[0])[:8]]
        assert flags == [1, 0, 1, 0, 1, 0, 1, 0]                # every other corner net has its adjacency planes on
    for s, which, binds in ts.BOUNDARY_CASES:
        fit, over, w = ts.boundary_net(s, which)
        assert over is not None and w == binds and len(over) == len(fit) + 1 <= 128 and over[:-1] == fit, (s, which, w)
        assert all(ts.net_fits(s, fit)[2:])
    assert ts.boundary_net((12, 34, 25), "s1")[2] == "s2"
