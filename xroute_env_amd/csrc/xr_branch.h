// xr_branch.h — branch (xr_batch_branch): env slots take other slots' state on the device.  Included by xr_kernels.hip after
// xr_rollout.h; no router source changes.
//
// Row i of a map takes the state of row parent[i]; every read sees the state BEFORE the call, whatever the map is (a swap, a cycle, a
// chain, a fan-out from a slot that is itself overwritten).  A slot that is overwritten may be someone's parent, so the copy cannot be one
// in-place launch.  Every row classifies itself from the map alone — its own entry and its parent's entry, no list, no counter:
//   keeper    parent[i] < 0 or == i: not written.
//   flagged   parent[i] >= rows: keeps its state, XR_ENV_BAD_ACTION is OR-ed into its status words (pass 1 writes them).
//   direct    its parent is a plain keeper: nobody writes the parent during this call.
//   staged    its parent is itself moved or flagged: pass 1 writes the parent.
//   xr_branch_kernel<0>   staged rows only: slot parent[i] -> staging row i.  Reads slots, writes staging.
//   xr_branch_kernel<1>   moved rows: slot parent[i] (direct) or staging row i (staged) -> slot i; flagged rows: the status bits.  Reads
//                         plain keepers and staging, writes moved and flagged slots.
// No launch both reads and writes a slot, and the two launches are ordered by the stream: no workgroup ever waits for another one, so
// branches of different env groups (each with a staging pool of its own) may share the chip in any interleaving.
// A streaming copy: workgroup (i, c) moves chunk c of row i's two long rows (owner, path) as 16-byte vectors; lane 0 of chunk 0 moves the
// scalars, loads first, then stores.
#pragma once

// bytes [0, n) from s to d (n a multiple of 4): this workgroup chunk's share.  16-byte vectors where both rows start on a 16-byte
// boundary (the owner rows always do: n_max is a multiple of 8 elements; the path rows do when path_cap % 4 == 0, or for a pair of rows
// that happens to) with a 4-byte tail; else 4-byte words throughout
__device__ __forceinline__ void xr_branch_copy_row(const void* __restrict__ s, void* __restrict__ d, const uint32_t n, const int t, const int nt) {
    const uint32_t words = n >> 2;
    uint32_t done = 0;
    if (((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d)) & 15) == 0) {
        const uint4* __restrict__ s4 = static_cast<const uint4*>(s);
        uint4* __restrict__ d4 = static_cast<uint4*>(d);
        const uint32_t nv = n >> 4;
        for (uint32_t k = t; k < nv; k += nt) d4[k] = s4[k];
        done = nv << 2;
    }
    const uint32_t* __restrict__ s1 = static_cast<const uint32_t*>(s);
    uint32_t* __restrict__ d1 = static_cast<uint32_t*>(d);
    for (uint32_t k = done + t; k < words; k += nt) d1[k] = s1[k];
}

// everything that is state of one slot: row sr of `s` to row dr of `d`
static_assert(sizeof(XrSlotRows) == 17 * sizeof(void*), "xr_branch_copy_slot moves 17 rows");   // a row added to XrSlotRows is moved here too, or branch drops it
__device__ __forceinline__ void xr_branch_copy_slot(const XrSlotRows& s, const int64_t sr, const XrSlotRows& d, const int64_t dr, const int n_max,
                                                    const int path_cap, const int words) {
    const int t = blockIdx.y * blockDim.x + threadIdx.x, nt = gridDim.y * blockDim.x;
    xr_branch_copy_row(s.owner + sr * n_max, d.owner + dr * n_max, (uint32_t)n_max * 2u, t, nt);
    xr_branch_copy_row(s.path + sr * path_cap, d.path + dr * path_cap, (uint32_t)path_cap * 4u, t, nt);
    if (t != 0) return;
    const int32_t nlegal = s.nlegal[sr], status = s.status[sr], path_len = s.path_len[sr], region = s.env_region[sr], replay = s.env_replay[sr];
    const int32_t sweeps = s.sweeps[sr], touched = s.touched[sr];
    const int32_t c0 = s.cum[3 * sr], c1 = s.cum[3 * sr + 1], c2 = s.cum[3 * sr + 2];
    const int32_t d0 = s.delta[3 * sr], d1 = s.delta[3 * sr + 1], d2 = s.delta[3 * sr + 2];
    const double reward = s.reward[sr];
    const uint8_t done = s.done[sr];
    const uint64_t hash = s.hash[sr];
    const int64_t env_steps = s.env_steps[sr];
    const uint4* __restrict__ rs = reinterpret_cast<const uint4*>(s.records + sr);      // 48 bytes, 16-byte aligned: three vectors
    const uint4 r0 = rs[0], r1 = rs[1], r2 = rs[2];
    d.nlegal[dr] = nlegal; d.status[dr] = status; d.path_len[dr] = path_len; d.env_region[dr] = region; d.env_replay[dr] = replay;
    d.sweeps[dr] = sweeps; d.touched[dr] = touched;
    d.cum[3 * dr] = c0; d.cum[3 * dr + 1] = c1; d.cum[3 * dr + 2] = c2;
    d.delta[3 * dr] = d0; d.delta[3 * dr + 1] = d1; d.delta[3 * dr + 2] = d2;
    d.reward[dr] = reward;
    d.done[dr] = done;
    d.hash[dr] = hash;
    d.env_steps[dr] = env_steps;
    uint4* __restrict__ rd = reinterpret_cast<uint4*>(d.records + dr);
    rd[0] = r0; rd[1] = r1; rd[2] = r2;
    for (int w = 0; w < words; w++) d.legal[dr * words + w] = s.legal[sr * words + w];
}

// env: the batch's rows (absolute slots; the map's row i is slot env_lo + i).  stg: the caller's staging pool, `rows` rows.
template <int PASS>
__global__ void __launch_bounds__(256) xr_branch_kernel(XrSlotRows env, XrSlotRows stg, int env_lo, int rows, const int32_t* __restrict__ parent,
                                                        int n_max, int path_cap, int words) {
    const int i = blockIdx.x;
    const int p = parent[i];
    if (p < 0 || p == i) return;                                   // keeper
    if (p >= rows) {                                               // flagged: the slot keeps its state
        if (PASS == 1 && blockIdx.y == 0 && threadIdx.x == 0) {
            env.status[env_lo + i] |= XR_ENV_BAD_ACTION;
            env.records[env_lo + i].status |= (uint16_t)XR_ENV_BAD_ACTION;
        }
        return;
    }
    const int q = parent[p];
    const bool staged = q >= 0 && q != p;                          // pass 1 writes the parent (moved, or flagged)
    if (PASS == 0) {
        if (staged) xr_branch_copy_slot(env, env_lo + p, stg, i, n_max, path_cap, words);
    } else if (staged) {
        xr_branch_copy_slot(stg, i, env, env_lo + i, n_max, path_cap, words);
    } else {
        xr_branch_copy_slot(env, env_lo + p, env, env_lo + i, n_max, path_cap, words);
    }
}
