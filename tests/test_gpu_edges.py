"""Edge cases of the domain on the GPU path: mixed region shapes in one batch, hundreds of nets (multi-word legal
bitmask), maximum layer count, path truncation, load-time limits and argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch

from xroute_env_amd.regions import ACCESS, NORMAL, Region, generate_region, pack_records

pytestmark = pytest.mark.gpu


def _episode_vs_oracle(regions, steps=400, **kw):
    from xroute_env_amd.batch import RegionBatch
    return _play_vs_oracle(RegionBatch(regions, device="cuda:0", **kw), steps)


def _play_vs_oracle(batch, steps=400):
    """Every slot of a loaded batch (slot e plays region e % n_regions, as after a load) from reset to its episode end."""
    from oracle import xr_oracle as orc
    envs = [orc.OracleEnv(batch.regions[e % len(batch.regions)]) for e in range(batch.n_envs)]
    batch.reset()
    obs = batch.alloc_observation()
    rng = np.random.default_rng(3)
    for _ in range(steps):
        legal = batch.legal_sets()
        if not any(legal):
            break
        acts = [int(rng.choice(sorted(s))) if s else 0 for s in legal]
        batch.step(torch.tensor(acts, dtype=torch.int32, device="cuda:0"), obs)
        delta = batch.fetch("delta").cpu().numpy()
        plen = batch.fetch("path_len").cpu().numpy()
        path = batch.fetch("path").cpu().numpy()
        status = batch.fetch("status").cpu().numpy()
        o = obs.cpu().numpy()
        for i, env in enumerate(envs):
            if not acts[i]:
                continue
            ref = env.step(acts[i], path_cap=batch.path_cap)
            assert delta[i].tolist() == ref["delta"].tolist() and status[i] == ref["status"]
            assert plen[i] == ref["path_len"] and path[i, :min(plen[i], batch.path_cap)].tolist() == ref["path"].tolist()
            ro = env.observation()
            assert np.array_equal(ro.ravel(), o[i, :ro.size])
    assert [int(h) for h in batch.fetch("hash").cpu().numpy().view(np.uint64)] == [e.hash() for e in envs]
    return batch


def test_mixed_region_shapes_in_one_batch():
    """Different (X, Y, Z) per region in the same batch: per-region strides, generic column pass, scalar and
    float4 observation paths side by side."""
    dims = [(24, 40, 9), (5, 7, 3), (12, 12, 12), (9, 4, 2), (1, 6, 1), (16, 16, 5)]
    regions = [generate_region(9700 + i, dims=d, k_range=(1, 6), net_span=5) for i, d in enumerate(dims)]
    _episode_vs_oracle(regions)


def test_hundreds_of_nets_multiword_legal_mask():
    reg = generate_region(9710, dims=(40, 40, 4), k_range=(200, 200), pins=(2, 2), aps=(1, 2), net_span=6,
                          blockage=(0.02, 0.04), prerouted=(0.0, 0.01))
    assert reg.n_nets > 128                       # > 2 words of the 64-bit legal bitmask
    b = _episode_vs_oracle([reg, reg], steps=40)
    assert b.legal_words >= 3


def test_maximum_layer_count_and_single_row_regions():
    regions = [generate_region(9720, dims=(6, 6, 32), k_range=(3, 3), net_span=3),
               generate_region(9721, dims=(1, 30, 2), k_range=(2, 2), net_span=10),
               generate_region(9722, dims=(30, 1, 2), k_range=(2, 2), net_span=10)]
    _episode_vs_oracle(regions)


def test_path_truncation_flag_and_exact_metrics():
    reg = generate_region(9730, dims=(24, 40, 9), k_range=(6, 6))
    b = _episode_vs_oracle([reg], path_cap=3)          # recorded path truncated, metrics and hash still exact
    assert b.path_cap == 3


def test_reload_changes_router_form():
    """One handle, reloaded from regions whose distance field fits LDS to one that takes the HBM-scratch form of the frontier router
    (64x48x12 = 36 864 nodes: 4 bytes a node plus the masks exceed the 160 KB of LDS) and back: every load replaces what the one before
    decided, and each plays bit-exact."""
    from xroute_env_amd.batch import RegionBatch
    small = [generate_region(9750 + i, dims=(6, 6, 2), k_range=(2, 3), net_span=4) for i in range(2)]
    large = [generate_region(9752, dims=(64, 48, 12), k_range=(4, 6), net_span=8)]
    assert large[0].n_nets <= 6
    batch = _play_vs_oracle(RegionBatch(small, n_envs=4, device="cuda:0"))
    lds = [batch.route_occupancy()[1]]
    for regions in (large, small):
        batch.regions = list(regions)
        with torch.cuda.device(batch.device):
            batch._load()
        lds.append(batch.route_occupancy()[1])
        assert batch.n_max == (max(r.n_nodes for r in regions) + 7) // 8 * 8
        _play_vs_oracle(batch)
    assert lds[0] != lds[1] and lds[1] != lds[2] and lds[2] == lds[0], lds
    assert lds[1] > 60 * 1024 > lds[0]       # the group table and work lists of the HBM-scratch form against a 72-node field


def _desc(L, reg):
    from xroute_env_amd import _lib
    d = _lib.XrRegionDesc()
    keep = [np.ascontiguousarray(reg.xs, np.int32), np.ascontiguousarray(reg.ys, np.int32),
            np.ascontiguousarray(reg.layer_dir, np.uint8), np.ascontiguousarray(reg.nodes, np.uint32)]
    d.dim_x, d.dim_y, d.dim_z = reg.dims
    d.xs_host, d.ys_host, d.layer_dir_host, d.nodes_host = (k.ctypes.data for k in keep)
    d.n_nets = reg.n_nets
    return d, keep


def test_load_time_limits_are_errors_not_crashes():
    from xroute_env_amd import _lib
    L = _lib.lib()
    cfg = _lib.default_config()
    h = C.c_void_p()
    assert L.xr_batch_create(C.byref(cfg), C.byref(h)) == 0
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = generate_region(9740, dims=(6, 6, 2), k_range=(2, 2))

    def load(reg):
        d, keep = _desc(L, reg)
        arr = (_lib.XrRegionDesc * 1)(d)
        return L.xr_batch_load_regions(h, arr, 1, stream)

    # a net with more access points than the kernel stages
    n = 20 * 20 * 2
    ntype = np.full(n, NORMAL); used = np.zeros(n, int); net = -np.ones(n, int); pin = -np.ones(n, int)
    ntype[:200] = ACCESS; net[:200] = 0; pin[:200] = np.arange(200) % 3
    many = Region((20, 20, 2), np.arange(20, dtype=np.int32) * 400, np.arange(20, dtype=np.int32) * 380,
                  np.array([0, 1], np.uint8), pack_records(ntype, used, net, pin), 1)
    assert load(many) == _lib.XR_ERR_RANGE and b"access points" in L.xr_last_error()
    # ACCESS node naming a net id beyond n_nets
    bad = Region(good.dims, good.xs, good.ys, good.layer_dir, good.nodes, 1)
    assert load(bad) == _lib.XR_ERR_RANGE
    # coordinates not strictly increasing
    flat = Region(good.dims, np.zeros(6, np.int32), good.ys, good.layer_dir, good.nodes, good.n_nets)
    assert load(flat) == _lib.XR_ERR_INVALID and b"strictly increasing" in L.xr_last_error()
    # too many layers
    tall = Region((2, 2, 33), np.arange(2, dtype=np.int32), np.arange(2, dtype=np.int32), np.zeros(33, np.uint8),
                  np.full(2 * 2 * 33, 1, np.uint32), 0)
    assert load(tall) == _lib.XR_ERR_RANGE
    # calls before a successful load
    acts = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    assert L.xr_batch_step(h, C.c_void_p(acts.data_ptr()), stream) == _lib.XR_ERR_STATE
    assert load(good) == 0
    assert L.xr_batch_fetch(h, 99, C.c_void_p(acts.data_ptr()), 4, stream) == _lib.XR_ERR_INVALID
    assert L.xr_batch_fetch(h, _lib.XR_FETCH_CUM, C.c_void_p(acts.data_ptr()), 4, stream) == _lib.XR_ERR_RANGE
    L.xr_batch_destroy(h)


def test_config_limits():
    from xroute_env_amd import _lib
    L = _lib.lib()
    for field, val in (("n_envs", 0), ("via_cost", 0), ("via_cost", 1 << 23), ("block_threads", 100), ("max_route_count", 0)):
        cfg = _lib.default_config()
        setattr(cfg, field, val)
        h = C.c_void_p()
        assert L.xr_batch_create(C.byref(cfg), C.byref(h)) < 0, field
    cfg = _lib.default_config()
    cfg.device = 99
    h = C.c_void_p()
    assert L.xr_batch_create(C.byref(cfg), C.byref(h)) == _lib.XR_ERR_HIP


@pytest.mark.gpu
def test_env_state_dump_and_restore_continues_bit_identically():
    """RegionBatch.state_dict() / load_state_dict() (xr_batch_fetch / xr_batch_store of the arrays that are the env state): a twin
    restored from a mid-episode dump — after resets, rotation and rejected actions — continues exactly like the original: records,
    owners, legal sets, hash chains, and the observation."""
    import numpy as np
    import torch
    from xroute_env_amd.batch import RegionBatch
    from xroute_env_amd.regions import generate_region
    regions = [generate_region(6100 + i, dims=(10, 9, 4), k_range=(2, 5), net_span=5) for i in range(6)]
    kw = dict(n_envs=16, device="cuda:0", auto_reset=True, max_route_count=2)
    a = RegionBatch(regions, **kw)
    a.reset(rotate=True)
    acts = torch.empty(16, dtype=torch.int32, device="cuda:0")
    for i in range(9):
        a.random_actions(70 + i, acts)
        if i == 4:
            acts[::3] = 99          # rejected actions are state too (status bits)
        a.step(acts)
    dump = a.state_dict()
    b = RegionBatch(regions, **kw)
    b.load_state_dict(dump)
    for k in RegionBatch._STATE:
        assert torch.equal(a.fetch(k), b.fetch(k)), k
    for i in range(12):
        a.random_actions(90 + i, acts)
        a.step(acts)
        b.step(acts)
        assert np.array_equal(a.records(), b.records())
    for k in RegionBatch._STATE:
        assert torch.equal(a.fetch(k), b.fetch(k)), k
    oa, ob, nl, reg = a.observation(), b.observation(), a.fetch("nlegal").cpu(), a.fetch("region").cpu()
    for e in range(16):           # (the buffers are torch.empty beyond an env's (2+7K)*N floats)
        n = (2 + 7 * int(nl[e])) * regions[int(reg[e])].n_nodes
        assert torch.equal(oa[e, :n], ob[e, :n])
    with pytest.raises(Exception):
        RegionBatch(regions[:3], n_envs=16, device="cuda:0").load_state_dict(dump)


@pytest.mark.gpu
def test_env_state_restore_is_validated():
    """xr_batch_store range-checks the arrays the kernels index with (region index, legal bits, nets-left count: XR_ERR_RANGE
    instead of a device fault in the next step), the dump carries a fingerprint of the regions + step-relevant config it belongs to, and
    the batch's env-step counter is part of the state."""
    import torch
    from xroute_env_amd import _lib
    from xroute_env_amd.batch import RegionBatch
    from xroute_env_amd.regions import generate_region
    regions = [generate_region(6200 + i, dims=(10, 9, 4), k_range=(2, 5), net_span=5) for i in range(6)]
    kw = dict(n_envs=8, device="cuda:0", auto_reset=True)
    a = RegionBatch(regions, **kw)
    a.reset()
    acts = torch.empty(8, dtype=torch.int32, device="cuda:0")
    for i in range(3):
        a.random_actions(5 + i, acts)
        a.step(acts)
    dump = a.state_dict()
    assert int(dump["steps"][0]) == a.total_steps() > 0
    b = RegionBatch(regions, **kw)
    b.load_state_dict(dump)
    assert b.total_steps() == a.total_steps()
    # a region index outside the loaded regions
    bad = dict(dump); bad["region"] = dump["region"].clone(); bad["region"][3] = len(regions)
    with pytest.raises(_lib.XRouteError) as ei:
        RegionBatch(regions, **kw).load_state_dict(bad)
    assert "region" in str(ei.value)
    # legal bits above the region's nets
    bad = dict(dump); bad["legal"] = dump["legal"].clone(); bad["legal"][2, 0] |= (1 << 40)
    with pytest.raises(_lib.XRouteError):
        RegionBatch(regions, **kw).load_state_dict(bad)
    bad = dict(dump); bad["nlegal"] = dump["nlegal"].clone(); bad["nlegal"][1] = 1000
    with pytest.raises(_lib.XRouteError):
        RegionBatch(regions, **kw).load_state_dict(bad)
    # same sizes, other content / other step-relevant config: refused by the fingerprint
    other = [generate_region(6300 + i, dims=(10, 9, 4), k_range=(2, 5), net_span=5) for i in range(6)]
    if max(r.n_nets for r in other) == max(r.n_nets for r in regions):
        with pytest.raises(ValueError):
            RegionBatch(other, **kw).load_state_dict(dump)
    with pytest.raises(ValueError):
        RegionBatch(regions, via_cost=900, **kw).load_state_dict(dump)
    #  all-or-nothing: a batch with a state of its own refuses a bad dump — whether the host check or the library's own range
    # check (host_checks=False: region stored first, then the library refuses `legal`) catches it — and keeps EXACTLY the state it had
    c = RegionBatch(regions, **kw)
    c.reset()
    c.random_actions(77, acts); c.step(acts)
    before = {k: c.fetch(k).clone() for k in RegionBatch._STATE}
    assert not torch.equal(before["owner"], a.fetch("owner"))
    bad = dict(dump); bad["legal"] = dump["legal"].clone(); bad["legal"][2, 0] |= (1 << 40)
    for host_checks in (True, False):
        with pytest.raises(_lib.XRouteError):
            c.load_state_dict(bad, host_checks=host_checks)
        for k in RegionBatch._STATE:
            assert torch.equal(c.fetch(k), before[k]), (k, host_checks)
    bad = dict(dump); bad["cum"] = dump["cum"][:-1]                      # a LATE array of the wrong shape: refused before anything moved
    with pytest.raises(ValueError):
        c.load_state_dict(bad)
    for k in RegionBatch._STATE:
        assert torch.equal(c.fetch(k), before[k]), k
    old = {k: v for k, v in dump.items() if k != "steps"}               # a dump from before `steps` was state: accepted, counter kept
    steps_c = c.total_steps()
    c.load_state_dict(old)
    assert c.total_steps() == steps_c and torch.equal(c.fetch("owner"), a.fetch("owner"))
    with pytest.raises(ValueError):
        c.load_state_dict({k: v for k, v in dump.items() if k != "hash"})
    # the batch that refused is still usable
    b.random_actions(9, acts); a.step(acts); b.step(acts)
    assert torch.equal(a.fetch("record"), b.fetch("record"))
