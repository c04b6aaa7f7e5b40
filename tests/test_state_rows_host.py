"""Host side of the packed-state sweep (tests/test_gpu_state_rows.py): the plain references of tests/state_rows.py against the CPU oracle and the
fixtures recorded from the reference's observation builder, proof that the case table can see the mistakes a packing kernel is likely to make, and the
exact set of shape classes the table puts in front of the kernels.  CPU only."""
import dataclasses
import inspect
import os
import struct

import numpy as np
import pytest

from oracle import xr_oracle as orc
from tests import state_rows as sr
from tests.helpers import g1_records, load_g1
from xroute_env_amd.regions import Region, unpack_records

M64 = 0xFFFFFFFFFFFFFFFF
IDS = [c.name for c in sr.CASES]


# ---- the references against the oracle and the reference's recorded observations -------------------------------------------------------------
def _played(region, seed):
    """An oracle env after a few nets routed in a seeded random order: up to three, one net is always left (the net planes need a legal net)"""
    steps = min(3, region.n_nets - 1)
    env = orc.OracleEnv(region)
    env.reset()
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        ids = env.legal()
        if not len(ids):
            break
        env.step(int(ids[rng.integers(len(ids))]))
    return env


@pytest.mark.parametrize("case", sr.CASES, ids=IDS)
def test_pack_then_expand_reproduces_the_oracles_head_planes_and_net_planes(case):
    """On routed states of every region of every case: ref_pack_row's legal mask is the oracle's legal list, ref_expand_row of that row is planes 0..1 of
    the oracle's observation (the same bits), and ref_net_planes of the first legal net is planes 2..8."""
    regions, sz = sr.case_regions(case), sr.sizes(case)
    for i, region in enumerate(regions):
        env = _played(region, case.seed + i)
        n, ids = region.n_nodes, env.legal()
        assert len(ids) > 0, (case.name, i)                     # (the net planes below need a legal net)
        obs = env.observation().reshape(2 + 7 * len(ids), n)
        owner = np.zeros(sz["n_max"], np.int16)
        owner[:n] = env.owner()
        row = sr.ref_pack_row(region, owner, ids, i, sz["legal_words"], sz["occ_words"], sz["row_bytes"] + 24)
        assert len(row) == sz["row_bytes"] + 24 and row[sz["row_bytes"]:] == bytes(24)
        assert struct.unpack("<4i", row[:16]) == (i, len(ids), sz["legal_words"], sz["occ_words"])
        assert sr.mask_ids(int.from_bytes(row[16:16 + 8 * sz["legal_words"]], "little")) == ids.tolist()
        head, nl, rg = sr.ref_expand_row(regions, row, sz["legal_words"], 2 * sz["n_max"])
        assert (nl, rg) == (len(ids), i) and head.dtype == np.float32
        assert np.array_equal(head.view(np.uint32), obs[:2].ravel().view(np.uint32)), (case.name, i)
        assert np.array_equal(sr.ref_net_planes(region, int(ids[0])).view(np.uint32), obs[2:9].view(np.uint32)), (case.name, i)
        for bad in (0, -1, region.n_nets + 1):
            assert not sr.ref_net_planes(region, bad).any()


def test_the_references_reproduce_the_observations_recorded_from_the_reference():
    """tests/golden/g1_build3dgrid.npz holds what the reference's build_3Dgrid returned for its `data` lists: planes 0..1 through ref_pack_row and
    ref_expand_row (owner = the records' is_used flag), planes 2 + 7 i .. 8 + 7 i through ref_net_planes of the i-th net of its netSet."""
    seen = 0
    for c in load_g1():
        X, Y, Z = (int(v) for v in c["dims"])
        n, nets = X * Y * Z, [int(v) for v in c["netset"]]
        if n == 0:
            continue
        rec = g1_records(c)
        used = unpack_records(rec)[1]
        region = Region((X, Y, Z), np.arange(X, dtype=np.int32), np.arange(Y, dtype=np.int32), (np.arange(Z) & 1).astype(np.uint8), rec, 0)
        region = dataclasses.replace(region, n_nets=max(nets + [int(sr.node_nets(region).max(initial=0))]))
        obs = c["obs_i16"].astype(np.float32).reshape(2 + 7 * len(nets), n)
        lw, ow = max(1, (region.n_nets + 63) // 64), (n + 63) // 64
        row = sr.ref_pack_row(region, used.astype(np.int16), nets, 0, lw, ow, sr.payload_bytes(lw, ow))
        head, nl, _ = sr.ref_expand_row([region], row, lw, 2 * n)
        assert nl == len(nets) and np.array_equal(head, obs[:2].ravel())
        for i, a in enumerate(nets):
            assert np.array_equal(sr.ref_net_planes(region, a), obs[2 + 7 * i:9 + 7 * i]), (seen, a)
        seen += 1
    assert seen >= 3


def test_expand_reference_refuses_what_the_header_says_it_refuses():
    case = sr.CASE_BY_NAME["n65"]
    regions, sz = sr.case_regions(case), sr.sizes(case)
    good = sr.case_rows(case, 0)[1]
    assert sr.ref_expand_row(regions, good, 1, 144)[2] == 0

    def hdr(row, **kw):
        f = dict(zip("r nl lw ow".split(), struct.unpack("<4i", row[:16])))
        f.update(kw)
        return struct.pack("<4i", f["r"], f["nl"], f["lw"], f["ow"]) + row[16:]

    for bad in (hdr(good, r=-1), hdr(good, r=1), hdr(good, lw=-1), hdr(good, lw=2), hdr(good, ow=-1), hdr(good, ow=1), hdr(good, ow=3),
                hdr(good, nl=struct.unpack("<4i", good[:16])[1] + 1)):
        assert sr.ref_expand_row(regions, bad, 1, 144) == (None, -1, -1)
    assert sr.ref_expand_row(regions, good, 1, 129) == (None, -1, -1)          # 2 N = 130 floats do not fit
    assert sr.ref_expand_row(regions, good + bytes(8), 1, 130)[2] == 0 and sz["occ_words"] == 2


# ---- the table can see mistakes -------------------------------------------------------------------------------------------------------------
def _occ_of(row, lw, ow):
    return bytearray(row[16 + 8 * lw:16 + 8 * (lw + ow)])


def _with_occ(row, lw, ow, occ):
    return row[:16 + 8 * lw] + bytes(occ) + row[16 + 8 * (lw + ow):]


def mutant_row(kind, region, owner, ids, r, lw, ow, rb):
    """ref_pack_row with one deliberate mistake"""
    row = sr.ref_pack_row(region, owner, ids, r, lw, ow, rb)
    n = region.n_nodes
    if kind == "no_tail_mask":          # the last chunk of eight nodes is taken whole: the owner row's padding counts
        m = sr.occupancy_mask(region, owner)
        for f in range(n, min((n + 7) & ~7, len(owner), 64 * ow)):
            m |= int(owner[f] != 0) << f
        return _with_occ(row, lw, ow, m.to_bytes(8 * ow, "little"))
    if kind == "bit_reversed":          # node f at bit 7 - f % 8 of its byte
        return _with_occ(row, lw, ow, bytes(int(f"{b:08b}"[::-1], 2) for b in _occ_of(row, lw, ow)))
    if kind == "byte_reversed":         # the bytes of every word in the other order
        occ = _occ_of(row, lw, ow)
        return _with_occ(row, lw, ow, b"".join(bytes(occ[8 * w:8 * w + 8][::-1]) for w in range(ow)))
    if kind == "node64_word0":          # the first node of word 1 lands on bit 0 of word 0
        m = int.from_bytes(_occ_of(row, lw, ow), "little")
        if (m >> 64) & 1:
            m = (m & ~(1 << 64)) | 1
        return _with_occ(row, lw, ow, m.to_bytes(8 * ow, "little"))
    if kind == "legal_bit_id":          # bit id instead of bit id - 1
        m = (sr.legal_mask(ids) << 1) & ((1 << (64 * lw)) - 1)
        return row[:16] + m.to_bytes(8 * lw, "little") + row[16 + 8 * lw:]
    raise KeyError(kind)


def cut_word(k, lo, word, kind="right"):
    """One word of the legal mask (bits lo .. lo + 63) cut to a region of k nets, word by word as a 64-bit kernel has to do it, right or with one deliberate
    mistake.  (A 64-bit shift takes its count modulo 64.)"""
    k = {"cut_k_plus_1": k + 1, "cut_k_minus_1": k - 1}.get(kind, k)
    whole = k > lo + 64 if kind == "gt_for_ge" else k >= lo + 64
    allowed = M64 if whole else (((1 << ((k - lo) & 63)) - 1) & M64 if k > lo else 0)
    return word & allowed


def mutant_expand_occ_offset(regions, row, learner_lw, head_stride):
    """ref_expand_row that looks for the occupancy words behind the LEARNER's legal words instead of the row's own"""
    _, _, lw, ow = struct.unpack("<4i", row[:16])
    shifted = row[:16 + 8 * lw] + row[16 + 8 * learner_lw:] + bytes(8 * (learner_lw - lw))
    return sr.ref_expand_row(regions, shifted, learner_lw, head_stride)


def _row_mutant_catchers(kind):
    out = set()
    for case in sr.CASES:
        regions, er, sz = sr.case_regions(case), sr.env_regions(case), sr.sizes(case)
        for t in range(sr.ROUNDS):
            rnd, rows = sr.case_rounds(case)[t], sr.case_rows(case, t)
            for e in range(case.n_envs):
                got = mutant_row(kind, regions[er[e]], rnd["owner"][e], rnd["want"][e]["ids"], er[e], sz["legal_words"], sz["occ_words"], sz["row_bytes"])
                if got != rows[e]:
                    out.add(case.name)
    return out


@pytest.mark.parametrize("kind,named", [("no_tail_mask", "n63"), ("bit_reversed", "n64"), ("byte_reversed", "n64"), ("node64_word0", "n65"),
                                         ("legal_bit_id", "k_all")])
def test_a_wrong_packing_gives_another_row_on_a_named_case(kind, named):
    caught = _row_mutant_catchers(kind)
    assert named in caught, (kind, sorted(caught))
    if kind == "no_tail_mask":          # only regions whose last chunk is part padding can tell; every such case does
        assert caught == {c.name for c in sr.CASES if True in sr.classes(c)["tail_chunk"]}
    if kind == "node64_word0":          # needs a node 64: every case but the three of one word
        assert caught == {c.name for c in sr.CASES} - {"n63", "n64", "n60"}


def test_the_word_by_word_cut_is_the_references_cut_and_each_wrong_cut_shows_on_a_named_case():
    catchers = {k: set() for k in ("cut_k_plus_1", "cut_k_minus_1", "gt_for_ge")}
    for case in sr.CASES:
        regions, er = sr.case_regions(case), sr.env_regions(case)
        for rnd in sr.case_rounds(case):
            for e in range(case.n_envs):
                k, words = regions[er[e]].n_nets, [int(w) for w in rnd["legal"][e]]
                assert [cut_word(k, 64 * w, v) for w, v in enumerate(words)] == rnd["want"][e]["legal"]
                for kind in catchers:
                    if [cut_word(k, 64 * w, v, kind) for w, v in enumerate(words)] != rnd["want"][e]["legal"]:
                        catchers[kind].add(case.name)
    assert "k1_63_64" in catchers["cut_k_plus_1"] and "k_all" in catchers["cut_k_plus_1"]
    assert "k1_63_64" in catchers["cut_k_minus_1"] and "n63" in catchers["cut_k_minus_1"]
    # `>` for `>=` is wrong only where a region's nets end with a word: K = 64 and K = 128
    assert catchers["gt_for_ge"] == {"k1_63_64", "k65_128", "k_all"}


def test_reading_the_occupancy_behind_the_learners_legal_words_shows_on_every_case():
    """The learner of the GPU sweep has more legal words than any sender; an expander that skips ITS count of words finds other occupancy bits"""
    caught = set()
    for case in sr.CASES:
        regions, sz = sr.case_regions(case), sr.sizes(case)
        lw_learner, stride = sz["legal_words"] + 1, 2 * sz["n_max"]
        for t in range(sr.ROUNDS):
            for row in sr.case_rows(case, t, row_bytes=sz["row_bytes"] + 8):
                want, got = sr.ref_expand_row(regions, row, lw_learner, stride), mutant_expand_occ_offset(regions, row, lw_learner, stride)
                assert want[0] is not None
                if got[0] is None or not np.array_equal(want[0], got[0]):
                    caught.add(case.name)
    assert caught == {c.name for c in sr.CASES}


# ---- the table is complete ------------------------------------------------------------------------------------------------------------------
# The kernels' loop bounds and path conditions, restated from csrc/xr_kernels.hip and csrc/xr_peek.h (quoted: the line each step comes from)
def kernel_pack_trips(n_max, threads):
    ow = (n_max + 63) >> 6                                  # "const int ow = (b.n_max + 63) >> 6;"
    nchunk = ow << 3                                        # "const int nchunk = ow << 3;"
    bound = (nchunk + threads - 1) // threads * threads     # "c < ((nchunk + 255) & ~255)" / "c < (nchunk + bdim - 1) / bdim * bdim"
    return bound // threads                                 # "c += 256" / "c += bdim"


def kernel_tail_masked(n):
    return any(n - (c << 3) < 8 for c in range((n + 7) >> 3))       # "const int left = R.N - (c << 3); if (left < 8) bits &= ..."


def kernel_store_path(n, aligned):
    return "vector" if aligned and (n & 3) == 0 else "scalar"      # "if (vec4 && (N & 3) == 0)" (expand and net_planes)


def kernel_vector_trips(n):
    return len(range(0, n, 1024))                           # "for (int f0 = tid * 4; f0 < N; f0 += 1024)" / "f0 += 256 * 4"


def kernel_cut_branch(k, lo):
    return "whole" if k >= lo + 64 else "part" if k > lo else "none"      # "K >= lo + 64 ? ~0ULL : (K > lo ? ((1ULL << (K - lo)) - 1ULL) : 0ULL)"


def test_the_table_holds_exactly_these_classes():
    assert len({c.name for c in sr.CASES}) == len(sr.CASES)
    union = {}
    for case in sr.CASES:
        regions, sz, cl = sr.case_regions(case), sr.sizes(case), sr.classes(case)
        assert case.n_envs <= 32 and max(r.n_nodes for r in regions) < 9000
        # the table's own class functions agree with the kernels' conditions
        assert cl["pack_passes"] == {kernel_pack_trips(sz["n_max"], 256)} and cl["peek_passes"] == {kernel_pack_trips(sz["n_max"], 1024)}
        assert cl["tail_chunk"] == {kernel_tail_masked(r.n_nodes) for r in regions}
        assert cl["store_path"] == {kernel_store_path(r.n_nodes, True) for r in regions}
        assert {kernel_store_path(r.n_nodes, False) for r in regions} == {"scalar"}
        assert cl["expand_passes"] == {kernel_vector_trips(r.n_nodes) for r in regions}
        for key, v in cl.items():
            union.setdefault(key, set()).update(v)
        union.setdefault("n", set()).update(r.n_nodes for r in regions)
        union.setdefault("cut", set()).update((w, kernel_cut_branch(r.n_nets, 64 * w)) for r in regions for w in range(sz["legal_words"]))
        union.setdefault("n_max_mod64", set()).add(sz["n_max"] % 64)
    assert union["n"] == {60, 63, 64, 65, 105, 600, 1024, 2048, 2052, 8192, 8228}
    assert union["n_mod64"] == {0, 1, 4, 24, 36, 41, 60, 63}            # 63, 64 and 65 themselves: bit 62 last, a word exactly, one bit of word 1
    assert union["n_mod8"] == {0, 1, 4, 7} and union["n_mod4"] == {0, 1, 3}
    assert union["store_path"] == {"vector", "scalar"} and union["tail_chunk"] == {True, False}
    assert union["pack_passes"] == {1, 2, 4, 5}                         # 2048 nodes fill one pass of 256 lanes; 2052 (n_max 2056, 33 words) need a second
    assert union["peek_passes"] == {1, 2}                               # 8192 nodes fill one pass of 1024 lanes; 8228 (129 words) need a second
    assert union["expand_passes"] == {1, 2, 3, 8, 9}
    assert union["legal_words"] == {1, 2, 3} and {1, 63, 64, 65, 128, 129} <= union["k"]
    assert union["cut"] == {(0, "part"), (0, "whole"), (1, "none"), (1, "part"), (1, "whole"), (2, "none"), (2, "part")}
    # the mixed batch: regions smaller than the rows, rows that do not end with a word, the largest region not the first
    mixed = sr.CASE_BY_NAME["mixed"]
    ns = [r.n_nodes for r in sr.case_regions(mixed)]
    assert sr.classes(mixed)["short_row"] == {60, 63, 105, 600} and sr.sizes(mixed)["n_max"] % 64 == 8 and ns.index(max(ns)) == 1
    assert all(not sr.classes(c)["short_row"] for c in sr.CASES if c is not mixed)
    # exact pass boundaries named by N
    for n, threads, trips in ((2048, 256, 1), (2052, 256, 2), (8192, 1024, 1), (8228, 1024, 2)):
        assert kernel_pack_trips((n + 7) & ~7, threads) == trips


def test_every_region_meets_every_pattern_it_can_tell_apart():
    """Per region of every case: all eight legal patterns (they depend on K); per case: all eleven occupancy patterns, and in the mixed batch per region
    (they depend on N).  The single nodes and ids that a region does not have are really put into the padding / beyond K, and the metrics move both ways."""
    for case in sr.CASES:
        er, nr = sr.env_regions(case), len(case.specs)
        occ = {r: set() for r in range(nr)}
        leg = {r: set() for r in range(nr)}
        for t in range(sr.ROUNDS):
            for e in range(case.n_envs):
                p = sr.pattern_index(case, e, t)
                occ[er[e]].add(sr.OCC_PATTERNS[p % len(sr.OCC_PATTERNS)])
                leg[er[e]].add(sr.LEGAL_PATTERNS[p % len(sr.LEGAL_PATTERNS)])
        assert all(v == set(sr.LEGAL_PATTERNS) for v in leg.values()), case.name
        assert set().union(*occ.values()) == set(sr.OCC_PATTERNS), case.name
        if case.name == "mixed":
            assert all(v == set(sr.OCC_PATTERNS) for v in occ.values())
        deltas = np.array([w["delta"] for rnd in sr.case_rounds(case) for w in rnd["want"]])
        assert (deltas < 0).any() and (deltas > 0).any() and np.abs(deltas).max() < 2 ** 31
        assert any(w["done"] for rnd in sr.case_rounds(case) for w in rnd["want"]) and any(not w["done"] for rnd in sr.case_rounds(case) for w in rnd["want"])
    # n63: the f63 and f64 singles and the whole `padding` pattern lie behind the region; ingest input bits beyond K exist where the words have room
    c63 = sr.CASE_BY_NAME["n63"]
    behind = [rnd["owner"][e][63:] for rnd in sr.case_rounds(c63) for e in range(c63.n_envs)]
    assert sum(bool(b.any()) for b in behind) >= 3
    for case in sr.CASES:
        regions, er = sr.case_regions(case), sr.env_regions(case)
        beyond = [int(w) != v for rnd in sr.case_rounds(case) for e in range(case.n_envs) for w, v in zip(rnd["legal"][e], rnd["want"][e]["legal"])]
        assert any(beyond), case.name
        assert all(len(w["ids"]) == w["nlegal"] and (not w["ids"] or w["ids"][-1] <= regions[er[e]].n_nets)
                   for rnd in sr.case_rounds(case) for e, w in enumerate(rnd["want"]))


def test_the_sweep_has_no_skips_or_expected_failures():
    here = os.path.dirname(os.path.abspath(__file__))
    words = ("skip", "xfail")
    for name in ("state_rows.py", "test_gpu_state_rows.py"):
        with open(os.path.join(here, name)) as f:
            text = f.read().lower()
        assert not any(w in text for w in words), name
    mod = inspect.getmodule(test_the_sweep_has_no_skips_or_expected_failures)        # (this file names the words: its marks are looked at instead)
    for name, fn in inspect.getmembers(mod, inspect.isfunction):
        assert all(m.name == "parametrize" for m in getattr(fn, "pytestmark", [])), name
    assert not hasattr(mod, "pytestmark")
