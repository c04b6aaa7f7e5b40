"""Shared helpers for the parity tests (fixture loading, reference-`data` conversion)."""
import hashlib
import json
import os

import numpy as np

from xroute_env_amd.regions import ACCESS, BLOCKAGE, NORMAL, Region, pack_records, records_from_entries

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def load_g1():
    z = np.load(os.path.join(GOLDEN, "g1_build3dgrid.npz"))
    cases = []
    for i in range(int(z["n_cases"])):
        p = f"c{i}_"
        cases.append({k[len(p):]: z[k] for k in z.files if k.startswith(p)})
    return cases


def g1_data(case) -> list:
    """Rebuild the reference `data` list of a G1 case."""
    nodes = [[[int(v) for v in m], [int(v) for v in p], [int(v) for v in t]]
             for m, p, t in zip(case["maze"], case["point"], case["info"])]
    return [[int(v) for v in case["dims"]], nodes, [int(v) for v in case["metrics"]],
            [int(v) for v in case["nets"]]]


def g1_records(case) -> np.ndarray:
    """Dense packed records of a G1 case (nodes absent from the list = unused NORMAL; a vertex listed twice = the reference's
    per-entry OR, regions.records_from_entries)."""
    X, Y, Z = (int(v) for v in case["dims"])
    n = X * Y * Z
    if not len(case["maze"]):
        return records_from_entries(n, [], [], [], [])
    m = case["maze"].astype(np.int64)
    info = case["info"].astype(np.int64)
    f = (m[:, 0] * Y + m[:, 1]) * Z + m[:, 2]
    return records_from_entries(n, f, info[:, 1], info[:, 0], info[:, 2])


def load_json(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


class OracleOrderSimulator:
    """CPU-oracle stand-in with xroute_env_amd.envs.order_contracts.OrderSimulator's interface: the checker the
    whole-order contracts (A3CGame / Route / OrderVectorEnv) are compared against.  Test infrastructure only."""

    def __init__(self, regions, n_envs=None, **oracle_kw):
        import torch
        from xroute_env_amd.proto import region_wire_fields
        self.torch = torch
        self.regions = list(regions)
        self.n_envs = int(n_envs if n_envs is not None else len(self.regions))
        self.device = torch.device("cpu")
        self.stride = max(max(r.n_nets for r in self.regions), 1)
        self.env_region = np.arange(self.n_envs) % len(self.regions)
        self.orders = torch.zeros((self.n_envs, self.stride), dtype=torch.int32)
        self.net_stats = torch.zeros((self.n_envs, self.stride, 4), dtype=torch.int32)
        self.batch = self                       # .batch.reset() of the GPU simulator
        self._wire = region_wire_fields
        self._kw = oracle_kw
        self.last = None

    def reset(self):
        pass

    def fields(self, r):
        return self._wire(self.regions[r])

    def assign(self, env_region):
        self.env_region = np.asarray(env_region, np.int64) % len(self.regions)

    def default_orders(self):
        o = self.torch.zeros((self.n_envs, self.stride), dtype=self.torch.int32)
        for e, r in enumerate(self.env_region):
            k = self.regions[r].n_nets
            o[e, :k] = self.torch.arange(1, k + 1, dtype=self.torch.int32)
        return o

    def route(self, orders, with_stats=True):
        from oracle.xr_oracle import OracleEnv
        cum = self.torch.zeros((self.n_envs, 3), dtype=self.torch.int32)
        self.last = []
        for e, r in enumerate(self.env_region):
            env = OracleEnv(self.regions[r], **self._kw)
            env.reset()
            status, plen = 0, 0
            for a in orders[e].tolist():
                if a <= 0 or env.nlegal() == 0:
                    break
                res = env.step(int(a))
                status |= res["status"]
                if not (res["status"] & 1):
                    plen += res["path_len"]
                    if with_stats:
                        self.net_stats[e, a - 1, :3] = self.torch.as_tensor(res["delta"])
                        self.net_stats[e, a - 1, 3] += 1
            cum[e] = self.torch.as_tensor(env.cum())
            self.last.append(dict(status=status, path_len=plen, owner=env.owner().copy(), done=env.nlegal() == 0))
        return cum


# ---- observation writers against the oracle (tests/test_gpu_obs_writers.py) ------------------------------------------------------
# The shapes the writers branch on.  dims -> N decides which unit writer runs (N % 4, N % 16), where a unit starts in its 16-byte
# slot and 128-byte line ((2 + 7 rank) N), whether planes 0..1 have a whole slot (2 N >= 16) and a unit a whole line (7 N >= 128).
OBS_SHAPE_SETS = {
    "tiny": [(1, 1, 1), (1, 3, 1), (1, 7, 1), (3, 1, 5), (17, 1, 1)],
    "sub_line": [(5, 7, 3), (7, 9, 2), (3, 43, 1), (11, 3, 4), (17, 2, 2)],
    "odd": [(7, 9, 5), (9, 11, 5), (15, 17, 9), (23, 15, 5)],
    "pack_like": [(25, 18, 17)],
    "aligned": [(16, 10, 4), (24, 40, 9)],
}
OBS_MIXED_FROM = ("aligned", "odd", "sub_line", "tiny")     # one region of each in one batch
OBS_MANY_NETS = dict(dims=(23, 15, 5), k_range=(200, 255), net_span=6, pins=(2, 2), aps=(1, 1))
OBS_SETS = tuple(OBS_SHAPE_SETS) + ("mixed", "many_nets", "exactly_255")
SENTINEL_F32, SENTINEL_U8 = -7.0, 0xAB


def obs_set_regions(name, seed=7000):
    """The regions of one row of the shape table (deterministic; at least one net each)."""
    from xroute_env_amd.regions import generate_region
    import dataclasses
    small = dict(k_range=(1, 9), net_span=4)
    if name in OBS_SHAPE_SETS:
        dims = OBS_SHAPE_SETS[name]
        reps = 2 if len(dims) > 2 else 3          # a few regions per shape: slots rotate to another region of another K
        return [generate_region(seed + i, dims=d, **small) for i in range(reps) for d in dims]
    if name == "mixed":
        return [generate_region(seed + i, dims=OBS_SHAPE_SETS[s][i % len(OBS_SHAPE_SETS[s])], **small)
                for i in range(2) for s in OBS_MIXED_FROM]
    if name == "many_nets":
        return [generate_region(seed + i, **OBS_MANY_NETS) for i in range(2)]
    if name == "exactly_255":
        # a region whose 255 nets all have access points (ids up to 255 in plane 1; sparse blockage leaves the generator the room),
        # the region of the 256-net refusal test with one net fewer (255 declared, a few with access points: only those are ever
        # legal), and a small one
        real = generate_region(seed, **dict(OBS_MANY_NETS, k_range=(255, 255), blockage=(0.02, 0.04), prerouted=(0.0, 0.01)))
        base = generate_region(seed + 1, dims=(23, 15, 5), **small)
        return [real, dataclasses.replace(base, n_nets=255), generate_region(seed + 2, dims=(7, 9, 5), **small)]
    raise KeyError(name)


def slot_records(region, owner_row):
    """The node records of a slot's CURRENT state: the region's static fields, is_used = the slot's owner array."""
    from xroute_env_amd.regions import pack_records, unpack_records
    ntype, _, net, pin = unpack_records(region.nodes)
    return pack_records(ntype, (owner_row[:region.n_nodes] != 0).astype(np.int64), net, pin)


def assert_rows_match_oracle(batch, buf, lo, hi, sentinel, full_write, what=""):
    """Rows of `buf` (row 0 = slot lo; fp32 or uint8) against oracle.build_observation of the state fetched from `batch`, slots [lo, hi):
    the first (2+7K)N values equal the oracle's (fp32: the same bits; uint8: the value as a byte); with `full_write` everything behind
    them, stride padding included, is still `sentinel`; without (an in-place step: older planes may remain up to the longest row)
    everything from (2 + 7 k_max) n_max on is.  Returns the region index of every slot checked."""
    from oracle import xr_oracle as orc
    reg = batch.fetch("region").cpu().numpy()
    owner = batch.fetch("owner").cpu().numpy()
    legal = batch.legal_sets()
    rows = buf.detach().cpu().numpy()
    u8 = rows.dtype == np.uint8
    assert u8 or rows.dtype == np.float32, rows.dtype
    assert rows.shape[0] >= hi - lo
    sent = np.array([sentinel], rows.dtype)
    bits = (lambda a: a) if u8 else (lambda a: a.view(np.uint32))
    longest = (2 + 7 * batch.k_max) * batch.n_max
    for e in range(lo, hi):
        region = batch.regions[int(reg[e])]
        ids = np.array(sorted(legal[e]), np.int32)
        want = orc.build_observation(region.dims, slot_records(region, owner[e]), ids).ravel()
        m = want.size
        assert m == (2 + 7 * ids.size) * region.n_nodes and m <= rows.shape[1], (what, e)
        if u8:
            assert (want == np.round(want)).all() and want.min(initial=0) >= 0 and want.max(initial=0) <= 255, (what, e)
            want = want.astype(np.uint8)
        row = rows[e - lo]
        bad = np.flatnonzero(bits(row[:m]) != bits(want))
        if bad.size:
            o = int(bad[0])
            raise AssertionError(f"{what}: slot {e} region {int(reg[e])} dims {region.dims} K {ids.size}: {bad.size} values differ, first at "
                                 f"offset {o} (plane {o // region.n_nodes}, node {o % region.n_nodes}): got {row[o]!r}, oracle {want[o]!r}")
        rest = row[m:] if full_write else row[max(m, longest):]
        bad = np.flatnonzero(bits(rest) != bits(sent)[0])
        if bad.size:
            o = int(bad[0]) + (m if full_write else max(m, longest))
            raise AssertionError(f"{what}: slot {e} region {int(reg[e])} dims {region.dims} K {ids.size}: {bad.size} values written behind the "
                                 f"row's {m} (first at offset {o}: {row[o]!r}, row length {row.size})")
    return [int(r) for r in reg[lo:hi]]
