"""Cases and plain references shared by the packed-state sweep (tests/test_gpu_state_rows.py, tests/test_state_rows_host.py): the packed row of an env
slot, its expansion into the two head planes, the ingest of an external state and the seven static planes of a net.  NumPy and Python integers only; no
GPU, no ctypes.  Written from the row layout documented at xr_batch_pack_state (include/xroute_hip.h) and from what the reference's observation builder
produces (baseline/build_3Dgrid.py), not from the kernels:

    row    = int32 region | int32 nlegal | int32 legal_words | int32 occ_words | uint64 legal[legal_words] | uint64 occ[occ_words]
    legal    bit id - 1 of the mask = net id is still to route; the mask is one integer cut into little-endian 64-bit words
    occ      bit f of the mask = node f (flat observation order, f = (x Y + y) Z + z) is an obstacle: a blockage, or held by anything

A row is stored little-endian, as the device holds it.  Everything here is deterministic: the GPU tests and the host tests rebuild the same inputs."""
import dataclasses
import functools
import struct

import numpy as np

from xroute_env_amd.regions import ACCESS, BLOCKAGE, generate_region, unpack_records

FOREIGN = 0x7FFF                # XR_OWNER_FOREIGN: a node held by a wire of no net of the region
W_VIOLATION, W_VIA, W_WIRELENGTH = 500, 4, 0.5      # the trainers' reward weights (baseline/DQN/train_DQN.py:98-99)
PACK_THREADS, PEEK_THREADS, NODES_PER_LANE = 256, 1024, 8      # the workgroups the two copies of the packing run with (peek: block_threads=1024)
EXPAND_STRIDE = 1024            # nodes per pass of the vector paths of expand and net_planes (256 lanes, four nodes each)


# ---- the references ------------------------------------------------------------------------------------------------------------------------
def node_nets(region) -> np.ndarray:
    """int64 [N]: -1 a blockage, 0 a plain node, the 1-based net id at an access point (the static half of a node record)"""
    ntype, _, net, _ = unpack_records(region.nodes)
    return np.where(ntype == BLOCKAGE, -1, np.where(ntype == ACCESS, net + 1, 0)).astype(np.int64)


def payload_bytes(legal_words: int, occ_words: int) -> int:
    return 16 + 8 * (legal_words + occ_words)


def occupancy_mask(region, owner) -> int:
    """bit f = node f is a blockage or owner[f] != 0, for f < N; owner may be longer than N (what lies behind N is padding and never counts)"""
    n = region.n_nodes
    used = (node_nets(region) == -1) | (np.asarray(owner)[:n] != 0)
    return int.from_bytes(np.packbits(used, bitorder="little").tobytes(), "little")


def legal_mask(ids) -> int:
    m = 0
    for i in ids:
        assert i >= 1
        m |= 1 << (int(i) - 1)
    return m


def mask_ids(mask: int) -> list:
    return [i + 1 for i in range(mask.bit_length()) if (mask >> i) & 1]


def ref_pack_row(region, owner, legal_ids, region_index, legal_words, occ_words, row_bytes) -> bytes:
    """The packed row of a slot that plays `region` with this owner row and these nets left.  `row_bytes` bytes: the payload, then zeros (the bytes
    behind the payload belong to the caller: compare payload_bytes(legal_words, occ_words) of them)."""
    need = payload_bytes(legal_words, occ_words)
    assert row_bytes >= need and row_bytes % 8 == 0, (row_bytes, need)
    ids = sorted(int(i) for i in legal_ids)
    row = struct.pack("<4i", int(region_index), len(ids), int(legal_words), int(occ_words))
    row += legal_mask(ids).to_bytes(8 * legal_words, "little")              # (OverflowError: an id the mask has no word for)
    row += occupancy_mask(region, owner).to_bytes(8 * occ_words, "little")  # (OverflowError: fewer than ceil(N / 64) words)
    return row + bytes(row_bytes - need)


def ref_expand_row(regions, row_bytes_blob, legal_words_of_learner, head_stride):
    """(head float32 [2 N], nlegal, region) of one row against the learner's region table, or (None, -1, -1) for a row the learner must refuse: a region
    index outside the table, a negative word count, more legal words than the learner has, words that do not fit the row, fewer occupancy bits than the
    region has nodes, planes that do not fit the head row, a nets-left count that is not the number of legal bits, a legal bit beyond the region's nets."""
    row = bytes(row_bytes_blob)
    refused = (None, -1, -1)
    r, nl, lw, ow = struct.unpack("<4i", row[:16])
    if not 0 <= r < len(regions):
        return refused
    if lw < 0 or lw > legal_words_of_learner or ow < 0 or payload_bytes(lw, ow) > len(row):
        return refused
    region = regions[r]
    n = region.n_nodes
    if ow * 64 < n or 2 * n > head_stride:
        return refused
    legal = int.from_bytes(row[16:16 + 8 * lw], "little")
    occ = int.from_bytes(row[16 + 8 * lw:16 + 8 * (lw + ow)], "little")
    ids = mask_ids(legal)
    if len(ids) != nl or (ids and ids[-1] > region.n_nets):
        return refused
    head = np.zeros(2 * n, np.float32)
    bits = np.unpackbits(np.frombuffer(occ.to_bytes(8 * ow, "little"), np.uint8), bitorder="little")
    head[:n] = bits[:n]
    k = min(len(ids), n)
    head[n:n + k] = ids[:k]
    return head, nl, r


def ref_ingest(region, prev_cum, owner, legal_words_in, cum) -> dict:
    """What a slot playing `region` reports after it adopts (owner, legal words, cumulative metrics): the legal words cut to the region's nets, their
    count, delta = new - previous cumulative metrics, the trainers' reward of that delta in double, done = no net left."""
    k = int(region.n_nets)
    words = [int(w) & 0xFFFFFFFFFFFFFFFF for w in legal_words_in]
    mask = sum(w << (64 * i) for i, w in enumerate(words)) & ((1 << k) - 1)
    legal = [(mask >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(len(words))]
    d = [int(c) - int(p) for c, p in zip(cum, prev_cum)]
    assert all(-2 ** 31 <= v < 2 ** 31 for v in d), d
    reward = -1 * (float(d[0]) * W_VIOLATION + float(d[2]) * W_VIA + float(d[1]) * W_WIRELENGTH)
    nlegal = bin(mask).count("1")
    return dict(legal=legal, ids=mask_ids(mask), nlegal=nlegal, delta=d, reward=reward, done=nlegal == 0,
                owner=np.asarray(owner)[:region.n_nodes].copy())


def ref_net_planes(region, net_id) -> np.ndarray:
    """float32 [7, N]: plane 0 = the access points of net `net_id` (1-based), planes 1..6 = those of them that have another access point of the net next to
    them along x, y or z (six identical planes: the reference fills one aliased array for its six directions).  An id that names no net: zeros."""
    X, Y, Z = (int(v) for v in region.dims)
    out = np.zeros((7, X * Y * Z), np.float32)
    if net_id <= 0 or net_id > region.n_nets:
        return out
    ap = (node_nets(region) == net_id).reshape(X, Y, Z)
    near = np.zeros_like(ap)
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        near[tuple(lo)] |= ap[tuple(hi)]
        near[tuple(hi)] |= ap[tuple(lo)]
    out[0] = ap.ravel()
    out[1:] = (ap & near).ravel()
    return out


# ---- the case table ------------------------------------------------------------------------------------------------------------------------
SMALL = dict(net_span=4)                                     # a few nets, up to four access points per pin: the adjacency planes are not empty
MANY = dict(net_span=6, pins=(2, 2), aps=(1, 1))             # many nets on a small grid (as the two-word test of test_gpu_learner_state.py)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    specs: tuple               # ((dims, (k_lo, k_hi), generator style), ...): one region each
    n_envs: int
    seed: int

    def __str__(self):
        return self.name


def _small(dims, k=(2, 6)):
    return (dims, k, "small")


def _many(k):
    return ((16, 16, 4), (k, k), "many")


# N = X Y Z of the dims used below: 7x3x3 = 63, 4x4x4 = 64, 13x5x1 = 65, 5x4x3 = 60, 7x5x3 = 105, 12x10x5 = 600, 16x16x8 = 2048, 19x12x9 = 2052,
# 32x32x8 = 8192, 22x22x17 = 8228, 16x16x4 = 1024
CASES = (
    Case("n63", (_small((7, 3, 3), (2, 4)),), 24, 9100),            # one bit short of a word: bit 63 of word 0 stays clear
    Case("n64", (_small((4, 4, 4), (2, 4)),), 24, 9110),            # one word exactly
    Case("n65", (_small((13, 5, 1), (2, 4)),), 24, 9120),           # node 64 = bit 0 of word 1; N % 4 = 1
    Case("n60", (_small((5, 4, 3), (2, 4)),), 24, 9130),            # N % 4 = 0, N % 8 = 4
    Case("n105", (_small((7, 5, 3)),), 24, 9140),                   # N % 4 = 1
    Case("n600", (_small((12, 10, 5)),), 24, 9150),                 # N % 8 = 0, N % 64 = 24
    Case("n2048", (_small((16, 16, 8)),), 24, 9160),                # one full pass of 256 lanes
    Case("n2052", (_small((19, 12, 9)),), 24, 9170),                # one chunk more: a second pass, and that chunk is half padding
    Case("n8192", (_small((32, 32, 8)),), 24, 9180),                # one full pass of 1024 lanes
    Case("n8228", (_small((22, 22, 17)),), 24, 9190),               # a second pass of 1024 lanes; N % 8 = 4
    Case("mixed", (_small((7, 5, 3)), _small((19, 12, 9)), _small((7, 3, 3), (2, 4)), _small((12, 10, 5)), _small((5, 4, 3), (2, 4))), 30, 9200),
    Case("k1_63_64", (_many(1), _many(63), _many(64)), 24, 9300),                                   # one legal word, the last one full
    Case("k65_128", (_many(65), _many(128)), 24, 9310),                                             # two legal words
    Case("k_all", (_many(1), _many(63), _many(64), _many(65), _many(128), _many(129)), 30, 9320),   # three: every branch of the cut in one batch
)
CASE_BY_NAME = {c.name: c for c in CASES}
ROUNDS = 2                      # successive ingests per case: the second one's deltas are taken against the first one's metrics

OCC_PATTERNS = ("free", "owned", "f0", "f7", "f8", "f63", "f64", "N-8", "N-1", "random", "padding")
LEGAL_PATTERNS = ("full", "empty", "id1", "id64", "id65", "idK", "random", "all_bits")


@functools.lru_cache(maxsize=None)
def case_regions(case: Case) -> tuple:
    """The regions of a case (shared: do not modify).  A spec with k_lo == k_hi must give exactly that many nets."""
    out = []
    for i, (dims, (k_lo, k_hi), style) in enumerate(case.specs):
        r = generate_region(case.seed + i, dims=dims, k_range=(k_lo, k_hi), **(SMALL if style == "small" else MANY))
        if not k_lo <= r.n_nets <= k_hi:
            raise AssertionError(f"case {case.name}: region {i} has {r.n_nets} nets, the table asks for {k_lo}..{k_hi}")
        out.append(r)
    return tuple(out)


def env_regions(case: Case) -> list:
    return [e % len(case.specs) for e in range(case.n_envs)]


def sizes(case: Case) -> dict:
    """What a batch of the case's regions must report: n_max (padded to 8 nodes), k_max, legal_words, occ_words, the smallest row"""
    regions = case_regions(case)
    n_max = (max(r.n_nodes for r in regions) + 7) & ~7
    k_max = max(r.n_nets for r in regions)
    lw, ow = max(1, (k_max + 63) // 64), (n_max + 63) // 64
    return dict(n_max=n_max, k_max=k_max, legal_words=lw, occ_words=ow, row_bytes=payload_bytes(lw, ow))


def pattern_index(case: Case, e: int, t: int) -> int:
    """Which occupancy and legal pattern slot e takes in round t: consecutive over the slots of one region, shifted by the region"""
    nr = len(case.specs)
    return e // nr + t * -(-case.n_envs // nr) + e % nr


def owner_row(case: Case, e: int, t: int) -> np.ndarray:
    """int16 [n_max]: the occupancy pattern of slot e in round t.  A single node that the region does not have (f >= N) is set all the same where the row
    has room for it: it lies in the padding and must not show.  `padding`: a free region and every element behind N set."""
    region = case_regions(case)[env_regions(case)[e]]
    n, n_max, k = region.n_nodes, sizes(case)["n_max"], max(region.n_nets, 1)
    rng = np.random.default_rng([case.seed, e, t, 1])
    values = np.where(rng.random(n_max) < 0.25, FOREIGN, rng.integers(1, k + 1, n_max)).astype(np.int16)
    row = np.zeros(n_max, np.int16)
    what = OCC_PATTERNS[pattern_index(case, e, t) % len(OCC_PATTERNS)]
    if what == "owned":
        row[:n] = values[:n]
    elif what == "random":
        pick = rng.random(n) < 0.3
        row[:n][pick] = values[:n][pick]
    elif what == "padding":
        row[n:] = values[n:]
    elif what != "free":
        f = {"f0": 0, "f7": 7, "f8": 8, "f63": 63, "f64": 64, "N-8": n - 8, "N-1": n - 1}[what]
        if 0 <= f < n_max:
            row[f] = values[f]
    return row


def legal_words_in(case: Case, e: int, t: int) -> list:
    """The legal words handed to ingest for slot e in round t (Python ints, one per legal word of the batch).  A single id above the region's nets is set
    all the same where the words have room for it; `all_bits` sets every bit of every word: ingest must cut both to the region's nets."""
    region = case_regions(case)[env_regions(case)[e]]
    k, lw = region.n_nets, sizes(case)["legal_words"]
    rng = np.random.default_rng([case.seed, e, t, 2])
    what = LEGAL_PATTERNS[pattern_index(case, e, t) % len(LEGAL_PATTERNS)]
    if what == "full":
        m = (1 << k) - 1
    elif what == "empty":
        m = 0
    elif what == "random":
        m = legal_mask(np.flatnonzero(rng.random(k) < 0.5) + 1)
    elif what == "all_bits":
        m = (1 << (64 * lw)) - 1
    else:
        i = {"id1": 1, "id64": 64, "id65": 65, "idK": k}[what]
        m = 1 << (i - 1) if 1 <= i <= 64 * lw else 0
    return [(m >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(lw)]


def cum_in(case: Case, e: int, t: int) -> list:
    """Cumulative (violation, wirelength, via) of slot e after round t: anywhere in [0, 2^30), so that deltas of both signs occur and each fits int32"""
    return [int(v) for v in np.random.default_rng([case.seed, e, t, 3]).integers(0, 1 << 30, 3)]


@functools.lru_cache(maxsize=None)
def case_rounds(case: Case) -> tuple:
    """Per round: dict(owner int16 [B, n_max], legal uint64 [B, legal_words], cum int32 [B, 3], want = [ref_ingest(...) per slot]).  The previous
    metrics of round 0 are the region's initial ones (what a reset leaves).  Shared: do not modify."""
    regions, er = case_regions(case), env_regions(case)
    prev = [[int(v) for v in regions[r].metrics0] for r in er]
    out = []
    for t in range(ROUNDS):
        owner = np.stack([owner_row(case, e, t) for e in range(case.n_envs)])
        legal = np.array([legal_words_in(case, e, t) for e in range(case.n_envs)], np.uint64)
        cum = np.array([cum_in(case, e, t) for e in range(case.n_envs)], np.int32)
        want = [ref_ingest(regions[er[e]], prev[e], owner[e], [int(w) for w in legal[e]], cum[e]) for e in range(case.n_envs)]
        prev = [[int(v) for v in cum[e]] for e in range(case.n_envs)]
        for a in (owner, legal, cum):
            a.setflags(write=False)
        out.append(dict(owner=owner, legal=legal, cum=cum, want=want))
    return tuple(out)


def case_rows(case: Case, t: int, region_base: int = 0, row_bytes=None, legal_words=None, occ_words=None) -> list:
    """ref_pack_row of every slot in the state round t leaves, in the batch's own word counts unless others are given"""
    sz = sizes(case)
    lw = sz["legal_words"] if legal_words is None else legal_words
    ow = sz["occ_words"] if occ_words is None else occ_words
    rb = payload_bytes(lw, ow) if row_bytes is None else row_bytes
    regions, er, rnd = case_regions(case), env_regions(case), case_rounds(case)[t]
    return [ref_pack_row(regions[er[e]], rnd["owner"][e], rnd["want"][e]["ids"], er[e] + region_base, lw, ow, rb) for e in range(case.n_envs)]


# ---- which path of which kernel a case takes, restated from the kernels' loop bounds ----------------------------------------------------------
def pack_passes(n_max: int, threads: int) -> int:
    """Trips of the packing loop: chunks of eight nodes of the whole row (occ_words words of eight chunks), one chunk per lane and pass"""
    return -(-(((n_max + 63) // 64) * 8) // threads)


def classes(case: Case) -> dict:
    """The shape classes a case puts in front of the kernels (sets over its regions / its batch)"""
    regions, sz = case_regions(case), sizes(case)
    ns = [r.n_nodes for r in regions]
    return dict(
        n_mod64={n % 64 for n in ns}, n_mod8={n % 8 for n in ns}, n_mod4={n % 4 for n in ns},
        store_path={"vector" if n % 4 == 0 else "scalar" for n in ns},                   # with an aligned buffer; unaligned: scalar for every N
        expand_passes={-(-n // EXPAND_STRIDE) for n in ns},
        pack_passes={pack_passes(sz["n_max"], PACK_THREADS)}, peek_passes={pack_passes(sz["n_max"], PEEK_THREADS)},
        tail_chunk={n % NODES_PER_LANE != 0 for n in ns},                                 # the last chunk of the region is masked
        short_row={n for n in ns if ((n + 7) & ~7) < sz["n_max"]},                        # regions smaller than the batch's rows
        legal_words={sz["legal_words"]}, k={r.n_nets for r in regions})
