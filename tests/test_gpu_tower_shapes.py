"""The fused towers (csrc/xr_agent.hip: `xr_agent_obstacle_tower` / agents.FusedObstacleTower, `xr_batch_net_vectors` / agents.FusedNetTower) over every
class of grid shape they accept, against an fp64 copy of the module on the CPU (tests/tower_shapes.py: weights, inputs, references, host predictions).
The other tower tests run six shapes with depth stride 2 or 3 against the framework's fp32 convolutions on the GPU; here: depth strides 1, 4, 5, 10, 11, 13
(gaps between the taps), strides 2 and 3 in h / w, od = 1 / 2 / 3, every strip width of the 1-channel block, LDS footprints at the limit, the net
tower's packed-coordinate limits (W = 32, H = 63, D = 32) and its list capacity at the boundary — in both matrix modes.  Bound: 2e-4 on the normalised
vectors (ts.TOL); every assertion message carries the measured error (table: LAB_NOTES.md)."""
import copy
import functools
import os
import subprocess
import sys

import pytest
import torch

from tests import tower_shapes as ts
from xroute_env_amd import agents

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_id = lambda s: "x".join(map(str, s))


@functools.lru_cache(maxsize=None)
def _rep(weights: str):
    return copy.deepcopy(ts.make_rep(weights)).to(DEV).eval()


def _err(got: torch.Tensor, ref: torch.Tensor) -> float:
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), (got.shape, ref.shape)
    return float((got.detach().double().cpu() - ref).abs().max())


def _report(what, err):
    print(f"TOWER_ERR {what} {err:.2e}")                    # (pytest -s: the table of LAB_NOTES.md)
    return err


def _head(shape, extra: int) -> torch.Tensor:
    """The sweep's five grids as rows of a head buffer whose stride is D H W rounded up to a multiple of four floats, + extra; 7.0 behind a row's grid"""
    n = shape[0] * shape[1] * shape[2]
    grids = ts.ob_grids(shape)
    head = torch.full((grids.shape[0], (n + 3) // 4 * 4 + extra), 7.0, dtype=torch.float32)
    head[:, :n] = grids
    return head.to(DEV)


# ---- 1. obstacle tower -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ts.OB_SHAPES, ids=_id)
def test_obstacle_tower_sweep(shape, monkeypatch):
    """One shape of the table in ts.OB_SHAPES: the kernel takes it (`supported` before and after every call: an XR_ERR_RANGE from the launcher would turn it
    off and let the framework path answer), the vectors are within 2e-4 of fp64, the same bits when run twice, the same bits from rows whose stride is no
    multiple of four floats (scalar loads instead of 16-byte ones), and within 2e-4 of fp64 with the 1-channel block's strip forced to 3, 4 and 5 cells per
    thread.
    The strips need NOT give the same bits, and do not (measured: normalised vectors up to 1.4e-6 apart).  xt_conv1_strips<3>, <5> and xt_conv1_pk4 add a
    cell's 27 products in the same (kd, kh, kw) order, but the source writes `acc += w * v` and leaves the fusing to the compiler: in the gfx950 code of the
    strips most cells are chains of v_fmac_f32, while the tail of some cells' sums is a v_pk_mul_f32 followed by two v_add_f32 (the product rounded before
    it is added) — which cells depends on the strip width.  Nothing needs more: the launcher picks the strip from the shape and the thread count alone, so the
    same shape in the same matrix mode always runs the same code (the run-twice and the odd-stride assertions), and XR_TOWER_STRIP is an A/B switch."""
    monkeypatch.delenv("XR_TOWER_STRIP", raising=False)
    ref = ts.ob_reference(shape)
    tower = agents.FusedObstacleTower(_rep("plain"), shape, DEV)
    assert tower.supported, shape
    head = _head(shape, 0)
    assert head.stride(0) % 4 == 0 and head.data_ptr() % 16 == 0
    got = tower(head)
    assert tower.supported, (shape, "the launcher refused the shape: the framework path answered")
    err = _report(f"obstacle {_id(shape)} mode1 strip=auto", _err(got, ref))
    assert err <= ts.TOL, (shape, err)
    assert torch.equal(got, tower(head)), shape
    odd = _head(shape, 1)
    assert odd.stride(0) % 4 == 1
    assert torch.equal(tower(odd), got), (shape, "rows of an odd stride")
    for strip in (3, 4, 5):
        monkeypatch.setenv("XR_TOWER_STRIP", str(strip))
        forced = tower(head)
        assert tower.supported, (shape, strip)
        e = _report(f"obstacle {_id(shape)} mode1 strip={strip}", _err(forced, ref))
        assert e <= ts.TOL, (shape, strip, e)
        assert torch.equal(forced, tower(head)), (shape, strip)


# ---- 2. net tower ------------------------------------------------------------------------------------------------------------------------
def _run_pairs(shape, weights, regions, what):
    """Every net of `regions` through the fused net tower: (vectors, the tower, the batch, the device pairs); asserts that no net fell back
    and that the planes built on the host from the access points are the ones the batch writes."""
    from xroute_env_amd.batch import RegionBatch
    D, H, W = shape
    batch = RegionBatch(list(regions), device=DEV)
    tower = agents.FusedNetTower(_rep(weights), shape, DEV)
    assert tower.supported, shape
    reg, net, planes = ts.pairs_of(regions)
    reg, net = reg.to(DEV), net.to(DEV)
    got = tower(batch, reg, net)
    assert tower.fallbacks == 0, (what, tower.fallbacks, "the framework path stood in for the kernel")
    mine = batch.net_planes(reg, net)[:, :7 * D * H * W].reshape(planes.shape).cpu()
    assert torch.equal(mine, planes), (what, "the host's net planes are not the batch's")
    return got, tower, batch, reg, net


@pytest.mark.parametrize("weights", ts.WEIGHT_SETS)
@pytest.mark.parametrize("shape", ts.NET_SHAPES, ids=_id)
def test_net_tower_sweep(shape, weights):
    """Every net of two generated regions of the shape (pin counts at which the host prediction says every net's lists fit: test_tower_shapes_host.py) with
    both weight sets: within 2e-4 of fp64 with NO net served by the framework path, the same bits twice, a sub-batch gives the rows of the whole batch."""
    what = f"net {_id(shape)} {weights} mode1"
    got, tower, batch, reg, net = _run_pairs(shape, weights, ts.net_regions(shape), what)
    err = _report(what, _err(got, ts.net_reference(shape, weights)))
    assert err <= ts.TOL, (what, err)
    assert torch.equal(got, tower(batch, reg, net)), what
    sel = torch.arange(1, reg.numel(), 3, device=DEV)
    assert torch.equal(tower(batch, reg[sel], net[sel]), got[sel]), what
    assert tower.fallbacks == 0
    batch.close()


# ---- 3. hand-built access points -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", ts.WEIGHT_SETS)
@pytest.mark.parametrize("shape", ts.HAND_SHAPES, ids=_id)
def test_net_tower_on_hand_built_access_points(shape, weights):
    """ts.hand_regions: (a) a net per corner of the tensor, every other one with its adjacency planes on (it also owns the corner's z neighbour in the region);
    (b) all eight corners in one net; (c) the whole first and last row (W = 32: mask words of all ones); (d) pairs 1, 2 and 5 apart along every axis; (e) 128
    access points in one block (the load limit).  The host prediction says every list fits, the kernel agrees (no fallback), every vector within 2e-4 of fp64."""
    regions, names = ts.hand_regions(shape)
    names = [n for nm in names for n in nm]
    what = f"hand {_id(shape)} {weights} mode1"
    got, tower, batch, reg, net = _run_pairs(shape, weights, regions, what)
    ref = ts.net_vectors64(weights, ts.pairs_of(regions)[2])
    errs = (got.double().cpu() - ref).abs().amax(dim=1).tolist()
    _report(what, _err(got, ref))
    bad = [(n, e) for n, e in zip(names, errs) if not e <= ts.TOL]
    assert not bad, (what, bad)
    assert torch.equal(got, tower(batch, reg, net)) and tower.fallbacks == 0, what
    batch.close()


@pytest.mark.parametrize("weights", ts.WEIGHT_SETS)
@pytest.mark.parametrize("shape,lattice,binds", ts.BOUNDARY_CASES, ids=lambda v: _id(v) if isinstance(v, tuple) else str(v))
def test_net_tower_list_capacity_boundary(shape, lattice, binds, weights):
    """(f) A scattered net grown point by point (ts.boundary_net) until the host says a list overflows — S1: (n1 + 1) // 2 + 7 n1 <= nB, S2: 6 D H + 1328 +
    (n2 + 1) // 2 + 7 n2 <= nC1, n1 / n2 = the access points dilated by one / two voxels.  The last net that fits goes through the kernel (fallbacks + 0),
    the first that does not is flagged and served by the framework path (fallbacks + exactly 1); both vectors within 2e-4 of fp64."""
    from xroute_env_amd.batch import RegionBatch
    fit, over, which = ts.boundary_net(shape, lattice)
    assert which == binds
    what = f"boundary {_id(shape)} {binds} {weights} mode1"
    regions = [ts.hand_region(shape, [fit]), ts.hand_region(shape, [over])]
    batch = RegionBatch(regions, device=DEV)
    tower = agents.FusedNetTower(_rep(weights), shape, DEV)
    assert tower.supported
    one = torch.ones(1, dtype=torch.int32, device=DEV)
    planes = ts.pairs_of(regions)[2]                          # (lattice points 3 apart in w are y neighbours in a region of 3 layers: some adjacency planes are on)
    assert torch.equal(batch.net_planes(torch.tensor([0, 1], device=DEV), torch.ones(2, dtype=torch.int32, device=DEV))[:, :planes[0].numel()].reshape(planes.shape).cpu(), planes)
    ref = ts.net_vectors64(weights, planes)
    v_fit = tower(batch, torch.tensor([0], device=DEV), one)
    assert tower.fallbacks == 0, (what, ts.net_fits(shape, fit), "the kernel refused a net the host prediction says fits")
    v_over = tower(batch, torch.tensor([1], device=DEV), one)
    assert tower.fallbacks == 1, (what, ts.net_fits(shape, over), "the kernel took a net the host prediction says does not fit")
    e_fit = _report(what + " fits", _err(v_fit, ref[:1]))
    e_over = _report(what + " falls-back", _err(v_over, ref[1:]))
    assert e_fit <= ts.TOL and e_over <= ts.TOL, (what, e_fit, e_over)
    batch.close()


# ---- 4. the fp32 matrix mode (fixed per process: one child with XR_TOWER_FP32=1) -------------------------------------------------------------
_FP32_CHILD = r"""
import copy, sys, torch
sys.path.insert(0, %r)
from xroute_env_amd import agents, _lib
from xroute_env_amd.batch import RegionBatch
from tests import tower_shapes as ts
dev = "cuda:0"
key = lambda s: "x".join(map(str, s))
out = {"mode": int(_lib.lib().xr_agent_matrix_mode())}
rep = copy.deepcopy(ts.make_rep("plain")).to(dev).eval()
for s in ts.OB_SHAPES:
    tower = agents.FusedObstacleTower(rep, s, dev)
    ok = bool(tower.supported)
    vec = tower(ts.ob_grids(s).to(dev))
    out["ob " + key(s)] = {"vec": vec.cpu(), "supported": ok and bool(tower.supported)}
for w in ts.WEIGHT_SETS:
    rep = copy.deepcopy(ts.make_rep(w)).to(dev).eval()
    for s in ts.NET_SHAPES:
        regions = ts.net_regions(s)
        batch = RegionBatch(list(regions), device=dev)
        tower = agents.FusedNetTower(rep, s, dev)
        reg, net, _ = ts.pairs_of(regions)
        vec = tower(batch, reg.to(dev), net.to(dev))
        out["net " + key(s) + " " + w] = {"vec": vec.cpu(), "supported": bool(tower.supported), "fallbacks": int(tower.fallbacks)}
        batch.close()
torch.save(out, sys.argv[1])
"""


@pytest.fixture(scope="module")
def fp32_mode(tmp_path_factory):
    """The shapes of parts 1 and 2 once more in ONE fresh process with XR_TOWER_FP32=1 (matrix mode 0: fp32 operands, 1024 threads — other strips, and the
    LDS limit of (14, 32, 22) to the byte); the child saves its vectors, the tests below hold them to the same fp64 references."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path_factory.mktemp("tower_fp32") / "vectors.pt")
    env = dict(os.environ, XR_TOWER_FP32="1")
    env.pop("XR_TOWER_STRIP", None)
    env.pop("XR_TOWER_THREADS", None)
    r = subprocess.run([sys.executable, "-c", _FP32_CHILD % root, path], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = torch.load(path)
    assert out["mode"] == 0
    return out


def test_this_process_runs_the_default_matrix_mode():
    from xroute_env_amd import _lib
    assert int(_lib.lib().xr_agent_matrix_mode()) == 1, "parts 1-3 are meant to cover matrix mode 1 (XR_TOWER_FP32 is set in this process)"


@pytest.mark.parametrize("shape", ts.OB_SHAPES, ids=_id)
def test_obstacle_tower_sweep_fp32_mode(shape, fp32_mode):
    got = fp32_mode["ob " + _id(shape)]
    assert got["supported"], (shape, "the launcher refused the shape in matrix mode 0")
    err = _report(f"obstacle {_id(shape)} mode0 strip=auto", _err(got["vec"], ts.ob_reference(shape)))
    assert err <= ts.TOL, (shape, err)


@pytest.mark.parametrize("weights", ts.WEIGHT_SETS)
@pytest.mark.parametrize("shape", ts.NET_SHAPES, ids=_id)
def test_net_tower_sweep_fp32_mode(shape, weights, fp32_mode):
    got = fp32_mode[f"net {_id(shape)} {weights}"]
    assert got["supported"] and got["fallbacks"] == 0, (shape, weights, got["supported"], got["fallbacks"])
    err = _report(f"net {_id(shape)} {weights} mode0", _err(got["vec"], ts.net_reference(shape, weights)))
    assert err <= ts.TOL, (shape, weights, err)
