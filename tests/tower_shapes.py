"""Inputs, fp64 references and host-side predictions shared by the tower shape sweep (tests/test_gpu_tower_shapes.py, its `XR_TOWER_FP32=1`
child process and tests/test_tower_shapes_host.py).  Everything here is deterministic and runs on the CPU: the GPU tests, the child and the host tests
rebuild the SAME weights, grids and regions from it.  Shapes are (D, H, W) of the observation tensor = (dim_z, dim_y, dim_x) of a region; a voxel
(d, h, w) of the tensor is node f = (d H + h) W + w of the region (the tensor is the node list reshaped)."""
import copy
import functools

import numpy as np
import torch

from xroute_env_amd import agents
from xroute_env_amd.regions import ACCESS, NORMAL, Region, generate_region, pack_records, unpack_records

TOL = 2e-4                      # the project's bound on normalised tower vectors (tests/test_agents.py), here against fp64

OB_SHAPES = [
    (3, 22, 24),                # sd = 1, od = 1, smallest D
    (5, 13, 22),                # od = 2; nB = 3080, the smallest accepted (limit 3072)
    (7, 34, 25),                # sd = 3, od = 2, (D - 3) % sd != 0
    (12, 34, 25),               # sd = 4: the 12-layer regions on the pack's common plane
    (12, 58, 17),               # sd = 4, 163 448 B of LDS
    (14, 32, 22),               # exactly 163 840 B by agents.FusedObstacleTower.accepts: with 1024 threads the launcher's limit to the byte
    (32, 19, 21),               # sd = 11: gaps between the depth taps
    (39, 12, 17),               # sd = 13, largest D
    (3, 63, 10),                # oh + 3 = 64
    (3, 129, 13),               # sh = 3
    (3, 13, 129),               # sw = 3
    (5, 15, 80),                # sw = 2, (W - 3) % sw != 0, W % 4 = 0
]
NET_SHAPES = [(3, 22, 24), (3, 17, 32), (5, 15, 19), (6, 52, 22), (12, 34, 25), (12, 58, 17), (9, 63, 5), (30, 7, 32), (32, 12, 17)]
HAND_SHAPES = [(3, 17, 32), (12, 34, 25)]
WEIGHT_SETS = ("plain", "skewed")
BOUNDARY_CASES = [((3, 17, 32), "s1", "s1"), ((3, 17, 32), "s2", "s2"), ((12, 34, 25), "s2", "s2")]      # (shape, lattice, the list that overflows first)


# ---- weights ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_rep(weights: str = "plain") -> agents.RepresentationNetwork:
    """A seeded RepresentationNetwork (CPU, fp32, eval mode) whose every BatchNorm has non-trivial statistics and affine parameters.  "skewed": on top of that
    one output channel of `net_align_conv1` and one of `net_conv1.conv2` is 30 x as large and another one of each 30 x smaller — the net tower derives the
    scale of its fixed-point scatters from the weights (XN_WSUM: a sum of per-tap maxima over the output channels), so the small channels are left with
    few of the 30 bits.  Shared between tests: do not modify (deepcopy it)."""
    assert weights in WEIGHT_SETS
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(11)
        rep = agents.RepresentationNetwork().eval()
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for m in rep.modules():
            if isinstance(m, torch.nn.BatchNorm3d):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=gen) * 0.2)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=gen) + 0.5)
                m.weight.copy_(torch.rand(m.weight.shape, generator=gen) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=gen) * 0.1)
        if weights == "skewed":
            for conv in (rep.net_align_conv1, rep.net_conv1.conv2):
                conv.weight[2] *= 30.0; conv.bias[2] *= 30.0
                conv.weight[5] /= 30.0; conv.bias[5] /= 30.0
    return rep


@functools.lru_cache(maxsize=None)
def make_rep64(weights: str = "plain") -> agents.RepresentationNetwork:
    """The fp64 reference module: a deepcopy of `make_rep` in double precision, on the plain path (3-D convolutions of the whole padded standard grid: none
    of the module's own shortcuts, which the host test holds to 1e-12 of this)."""
    rep64 = copy.deepcopy(make_rep(weights)).double().eval()
    rep64.crop_padding = rep64.fold_depth = rep64.fold_blocks = False
    return rep64


# ---- obstacle tower --------------------------------------------------------------------------------------------------------------------
def ob_grids(shape) -> torch.Tensor:
    """fp32 [5, D H W]: an empty grid, a full one, three random 0/1 grids of density 0.3"""
    D, H, W = shape
    gen = torch.Generator().manual_seed(100003 * D + 1009 * H + W)
    g = (torch.rand((5, D * H * W), generator=gen) < 0.3).float()
    g[0] = 0.0
    g[1] = 1.0
    return g


def ob_vectors64(shape, grids: torch.Tensor) -> torch.Tensor:
    D, H, W = shape
    with torch.no_grad():
        return agents.normalize(make_rep64().encode_obstacles(grids.double().reshape(-1, 1, D, H, W)))


@functools.lru_cache(maxsize=None)
def ob_reference(shape) -> torch.Tensor:
    """fp64 [5, 64] of `ob_grids(shape)` (computed once per process; do not modify)"""
    return ob_vectors64(shape, ob_grids(shape))


# ---- the towers' geometry and the net tower's list capacity, on the host ---------------------------------------------------------------
def geometry(shape) -> dict:
    D, H, W = shape
    sd, sh, sw = agents.align_stride(shape)
    od, oh, ow = (D - 3) // sd + 1, (H - 3) // sh + 1, (W - 3) // sw + 1
    return dict(sd=sd, sh=sh, sw=sw, od=od, oh=oh, ow=ow, nB=7 * od * oh * ow, nC1=21 * (oh + 3) * (ow + 3))


def dilated(shape, flat, r: int) -> int:
    """Voxels within r (Chebyshev) of one of the access points `flat`, clipped to the grid"""
    D, H, W = shape
    m = np.zeros(shape, bool)
    for f in flat:
        d, h, w = int(f) // (H * W), (int(f) // W) % H, int(f) % W
        m[max(d - r, 0): d + r + 1, max(h - r, 0): h + r + 1, max(w - r, 0): w + r + 1] = True
    return int(m.sum())


def net_fits(shape, flat):
    """(n1, n2, the S1 list fits, the S2 list fits): the kernel's lists of a net with these access points against the launcher's nB and nC1"""
    D, H, W = shape
    g = geometry(shape)
    n1, n2 = dilated(shape, flat, 1), dilated(shape, flat, 2)
    return n1, n2, (n1 + 1) // 2 + 7 * n1 <= g["nB"], 6 * D * H + 1328 + (n2 + 1) // 2 + 7 * n2 <= g["nC1"]


# ---- regions and their nets ------------------------------------------------------------------------------------------------------------
def region_nets(region: Region):
    """Per net (in id order): (node indices of its access points, ascending; 0/1 "has an axis neighbour in the REGION's (x, y, z) geometry that is an access
    point of the same net" — the reference's aliased direction planes, baseline/build_3Dgrid.py:125-138)"""
    X, Y, Z = region.dims
    ntype, _, net, _ = unpack_records(region.nodes)
    owner = np.where(ntype == ACCESS, net + 1, 0).reshape(X, Y, Z)
    pad = np.pad(owner, 1)
    same = np.zeros((X, Y, Z), bool)
    for ax in range(3):
        for s in (0, 2):
            sl = [slice(1, -1)] * 3
            sl[ax] = slice(s, s + (X, Y, Z)[ax])
            same |= (pad[tuple(sl)] == owner) & (owner > 0)
    owner, same = owner.reshape(-1), same.reshape(-1)
    out = []
    for k in range(1, region.n_nets + 1):
        f = np.flatnonzero(owner == k)
        out.append((f, same[f].astype(np.int64)))
    return out


def host_planes(shape, flat, adj) -> torch.Tensor:
    """fp32 [7, D, H, W]: plane 0 is 1 at the access points, planes 1..6 the access point's adjacency flag"""
    D, H, W = shape
    x = torch.zeros((7, D * H * W), dtype=torch.float32)
    f = torch.as_tensor(np.asarray(flat, np.int64))
    x[0, f] = 1.0
    x[1:, f] = torch.as_tensor(np.asarray(adj, np.float32))[None, :]
    return x.reshape(7, D, H, W)


def net_vectors64(weights: str, planes: torch.Tensor) -> torch.Tensor:
    """planes [n, 7, D, H, W] -> fp64 [n, 64]"""
    with torch.no_grad():
        return agents.normalize(make_rep64(weights).encode_nets(planes.double()))


def pairs_of(regions):
    """(region index int64 [n], 1-based net id int32 [n], planes fp32 [n, 7, D, H, W] built on the host) of every net of every region (one shape)"""
    X, Y, Z = regions[0].dims
    reg, net, planes = [], [], []
    for i, r in enumerate(regions):
        for k, (f, a) in enumerate(region_nets(r)):
            reg.append(i); net.append(k + 1); planes.append(host_planes((Z, Y, X), f, a))
    return torch.tensor(reg, dtype=torch.int64), torch.tensor(net, dtype=torch.int32), torch.stack(planes)


@functools.lru_cache(maxsize=None)
def net_regions(shape):
    """Two generated regions of at most 12 nets, with the largest pin counts of the generator at which the host prediction says every net's lists fit
    (shapes with a small first activation leave the S2 list little room: at (32, 12, 17) it holds 170 voxels, one access point; a second one, adjacent in the region's geometry, lies far away in the tensor's)."""
    D, H, W = shape
    for pins, aps in (((2, 4), (1, 4)), ((2, 3), (1, 2)), ((2, 2), (1, 2)), ((2, 2), (1, 1)), ((1, 1), (1, 1))):
        regions = [generate_region(7500 + i, dims=(W, H, D), k_range=(3, 12), pins=pins, aps=aps) for i in range(2)]
        if all(all(net_fits(shape, f)[2:]) for r in regions for f, _ in region_nets(r)):
            return tuple(regions)
    raise AssertionError(f"no generated region of shape {shape} fits the net tower's lists")


@functools.lru_cache(maxsize=None)
def net_reference(shape, weights: str) -> torch.Tensor:
    """fp64 [n, 64] of every net of `net_regions(shape)` in `pairs_of` order (computed once per process; do not modify)"""
    return net_vectors64(weights, pairs_of(net_regions(shape))[2])


def hand_region(shape, nets) -> Region:
    """A region of this tensor shape whose net k has exactly the access points nets[k] (node indices); every other node is a free NORMAL one"""
    D, H, W = shape
    N = D * H * W
    ntype = np.full(N, NORMAL, np.int64); net = np.full(N, -1, np.int64); pin = np.full(N, -1, np.int64)
    for k, f in enumerate(nets):
        f = np.asarray(sorted(int(v) for v in f), np.int64)
        assert len(set(f.tolist())) == len(f) and f.min() >= 0 and f.max() < N and (ntype[f] == NORMAL).all(), "access points must be distinct voxels"
        ntype[f] = ACCESS; net[f] = k; pin[f] = 0
    return Region((W, H, D), np.arange(W) * 400, np.arange(H) * 380, np.zeros(D, np.uint8), pack_records(ntype, np.zeros(N, np.int64), net, pin), len(nets))


def corners(shape):
    D, H, W = shape
    return [(d * H + h) * W + w for d in (0, D - 1) for h in (0, H - 1) for w in (0, W - 1)]


def hand_regions(shape):
    """The hand-built regions of the sweep's part 3 (a) .. (e): a list of regions and, per region, the name of every net"""
    D, H, W = shape
    fl = lambda d, h, w: (d * H + h) * W + w
    # (a) one net per corner; every other one also owns the corner's neighbour along the region's z axis (node f + 1: the next voxel of the tensor row), which is
    # what turns a net's adjacency planes on; (d) pairs 1, 2 and 5 apart along every axis that is long enough
    nets_a, names_a = [], []
    for i, c in enumerate(corners(shape)):
        on = i % 2 == 0
        nets_a.append([c, c + 1 if c % D < D - 1 else c - 1] if on else [c])
        names_a.append(f"corner{i}{'+adj' if on else ''}")
    i = 0
    for ax, n in enumerate(shape):
        for dist in (1, 2, 5):
            if dist + 1 > n:
                continue
            p = [0 if ax == 0 else D // 2, 3 + i, 2 + 2 * i]
            q = list(p)
            q[ax] += dist
            assert q[0] < D and q[1] < H and q[2] < W
            nets_a.append([fl(*p), fl(*q)]); names_a.append(f"pair axis {ax} dist {dist}")
            i += 1
    # (b) all eight corners in one net; (e) 128 access points (the load limit) in one block
    bd, bh, bw = (3, 6, 8) if D == 3 else (4, 4, 8)
    o = (0, 3, 3) if D == 3 else (2, 5, 5)
    block = [fl(o[0] + d, o[1] + h, o[2] + w) for d in range(bd) for h in range(bh) for w in range(bw)][:128]
    assert len(block) == 128
    # (c) the first and the last row of the tensor, whole (W = 32: mask words of all ones)
    rows = [fl(0, 0, w) for w in range(W)], [fl(D - 1, H - 1, w) for w in range(W)]
    return ([hand_region(shape, nets_a), hand_region(shape, [corners(shape), block]), hand_region(shape, list(rows))],
            [names_a, ["all corners", "block of 128"], ["first row", "last row"]])


def boundary_net(shape, which: str):
    """Part 3 (f): a scattered net grown point by point until the kernel's S1 (`which` = "s1") or S2 ("s2") list no longer fits.  Returns (the access points of
    the last net that fits, those of the first that does not — one more point, which of the two lists that one overflows).  The points are a shuffled
    lattice: 3 apart for "s1" (3x3x3 neighbourhoods side by side: the most S1 voxels per S2 voxel), 5 apart for "s2" (5x5x5 side by side), as far from the depth
    faces as the lattice allows for "s1" and on the first slice for "s2"."""
    D, H, W = shape
    step, off = (3, 1) if which == "s1" else (5, 2)

    def axis(n, first):                                     # lattice coordinates, plus the far face where the lattice's neighbourhoods stop short of it
        c = list(range(first, n, step))
        return c + [n - 1] if c[-1] + off < n - 1 else c
    pts = [(d * H + h) * W + w for d in axis(D, 1 if which == "s1" else 0) for h in axis(H, off) for w in axis(W, off)]
    rng = np.random.default_rng(17)
    pts = [pts[i] for i in rng.permutation(len(pts))][:128]
    for k in range(1, len(pts) + 1):
        n1, n2, f1, f2 = net_fits(shape, pts[:k])
        if not (f1 and f2):
            assert k > 1
            return pts[:k - 1], pts[:k], ("s1" if not f1 else "") + ("s2" if not f2 else "")
    return pts, None, ""
