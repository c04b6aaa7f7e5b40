// xr_tree_keep.h — kept trees (xr_batch_tree_search_keep, "XR-Tree v1, kept" of include/xroute_hip.h): the first kernel of a search that
// continues from the tree its caller's last kept call left.  Included by xr_kernels.hip after xr_tree.h; select, the rollout launch and
// backup of the call are xr_tree.h's, run on the half this kernel fills.  Clearing the outputs, the rebuilt root, the lookup of the
// played net's child and the expansion are xr_tree_core.h's; the key and the compaction are this file's own.
//
//   xr_tree_keep_begin_kernel   clears the row's outputs, checks the row's key against the env, then either copies the subtree below the
//                               played net from the old half into the new one (breadth first, returns shifted by the step's reward),
//                               copies the whole tree (the env has not moved), or builds the root as xr_tree_reset_kernel does; expands
//                               an unexpanded root; writes the new key and kept_out
// One wavefront per row.  The compaction goes level by level: the 64 lanes take the level's nodes in index order, a wave prefix sum over
// their child counts hands out the blocks, the lanes copy the children (64 at a time), and the next level is the range just written.  A
// copied node carries the OLD index of its block in `first` until its own level comes.  Nodes written by some lanes are read by others a
// level later: a workgroup barrier (one wave: a fence and no wait) stands between the levels.  Contraction is off in every function.
// The key check (xr_tree_keep_mode), the compaction (xr_tree_keep_compact) and the row's tree by its mode (xr_tree_keep_build) are device
// functions: xr_tree_eval_reopen_kernel (xr_tree_eval.h) runs the same ones on the evaluated search's pool.
#pragma once

// exclusive prefix sum of v over the wave; total: the sum of all 64
__device__ __forceinline__ int xr_tree_wave_offsets(const int v, const int lane, int& total) {
#pragma clang fp contract(off)
    int inc = v;
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    total = __shfl(inc, 63, 64);
    return inc - v;
}

// a node of the old frame in the new one: W' = W - (double)N * r, one multiplication, then one subtraction
__device__ __forceinline__ XrTreeNode xr_tree_shifted(XrTreeNode nd, const double r) {
#pragma clang fp contract(off)
    const double nr = (double)nd.N * r;
    nd.W = nd.W - nr;
    nd.V = 0;
    return nd;
}

// All 64 lanes: what becomes of a kept row.  0: rebuild; 1: the env has not moved (the whole tree); 2: the subtree below `child` of the
// old half.  a: the row's played entry (< 0: rebuild); key, klegal: the row's key and its legal words; legal, nl0, steps, region, replay:
// the env as it is now; n_add: the simulations the tree is about to take.  used_old: the old tree's nodes_used (read only where the key
// is looked at).  The same values in every lane.
__device__ __forceinline__ int xr_tree_keep_mode(const XrTreeNode* old, const XrTreeRow* rs, const XrTreeKey* key, const uint64_t* klegal,
                                                 const uint64_t* __restrict__ legal, const int words, const int a, const int nl0, const int64_t steps,
                                                 const int region, const int replay, const int node_cap, const int n_add, const int lane, int& child_out,
                                                 int& used_old_out) {
#pragma clang fp contract(off)
    int mode = 0, child = -1, used_old = 0;
    if (nl0 > 0 && a >= 0) {
        const XrTreeKey k = *key;
        bool ok = k.valid == 1 && k.region == region && k.replay == replay && k.env_steps + (a > 0 ? 1 : 0) == steps;
        const int aw = (a - 1) >> 6;
        const uint64_t abit = 1ull << ((a - 1) & 63);
        if (a > 0 && aw >= words) ok = false;
        int bad = 0;
        for (int wd = lane; wd < words; wd += 64) {
            uint64_t kw = klegal[wd];
            if (a > 0 && wd == aw) {
                if (!(kw & abit)) bad = 1;
                kw &= ~abit;
            }
            if (kw != legal[wd]) bad = 1;
        }
        if (__ballot(bad) != 0) ok = false;
        used_old = __builtin_amdgcn_readfirstlane(rs->used);
        if (ok && used_old >= 1 && used_old <= node_cap) {
            if (a == 0) {
                if ((int64_t)old[0].N + n_add <= XR_TREE_MAX_SIMS) mode = 1;
            } else {
                const int first = __builtin_amdgcn_readfirstlane(old[0].first);
                const int cnt = __builtin_amdgcn_readfirstlane(old[0].count);
                if (first >= 1 && cnt >= 1 && (int64_t)first + cnt <= used_old) {
                    const int found = xr_tree_child_by_net(old, first, cnt, a, lane);
                    if (found < cnt) {
                        child = first + found;
                        if ((int64_t)old[child].N + n_add <= XR_TREE_MAX_SIMS) mode = 2;
                    }
                }
            }
        }
    }
    child_out = __builtin_amdgcn_readfirstlane(child);
    used_old_out = used_old;
    return __builtin_amdgcn_readfirstlane(mode);
}

// All 64 lanes: the re-rooting.  The subtree below node `child` of `old` (a tree of used_old nodes) into `nodes`, breadth first, every
// node shifted by r; new node 0 is the old child with net 0 and P 1.  Returns the nodes written.  Ends with a workgroup barrier.
__device__ __forceinline__ int xr_tree_keep_compact(const XrTreeNode* old, XrTreeNode* nodes, const int child, const int used_old, const int node_cap,
                                                    const double r, const int lane) {
#pragma clang fp contract(off)
    if (lane == 0) {
        XrTreeNode nd = xr_tree_shifted(old[child], r);
        nd.P = 1.0; nd.net = 0;
        nodes[0] = nd;
    }
    __syncthreads();
    int lo = 0, hi = 1, nused = 1;
    while (lo < hi) {
        for (int base = lo; base < hi; base += 64) {
            const int idx = base + lane;
            int of = -1, cnt = 0;
            if (idx < hi) {
                of = nodes[idx].first;
                cnt = nodes[idx].count;
                if (of < 1 || cnt < 1 || (int64_t)of + cnt > used_old) { of = -1; cnt = 0; }
            }
            int total;
            int off = xr_tree_wave_offsets(cnt, lane, total);
            if (total > node_cap - nused) { of = -1; cnt = 0; off = 0; total = 0; }          // (never: the subtree is part of a tree that fitted)
            const int nf = nused + off;
            if (idx < hi) nodes[idx].first = of >= 0 ? nf : -1;
            uint64_t m = __ballot(cnt > 0);
            while (m) {
                const int p = __ffsll((long long)m) - 1;
                m &= m - 1;
                const int c_of = __shfl(of, p, 64), c_cnt = __shfl(cnt, p, 64), c_nf = __shfl(nf, p, 64);
                for (int c = lane; c < c_cnt; c += 64) nodes[c_nf + c] = xr_tree_shifted(old[c_of + c], r);
            }
            nused = __builtin_amdgcn_readfirstlane(nused + total);
        }
        __syncthreads();          // the level just written, before other lanes read it as parents
        lo = hi;
        hi = nused;
    }
    return nused;
}

// All 64 lanes: the tree of a kept call's row by its mode, into `v` (the half the call searches in), and what kept_out reports of it.
// r: the slot's reward row (read for mode 2 alone).  Ends with a workgroup barrier.
__device__ __forceinline__ void xr_tree_keep_build(const XrTreeView& v, const XrTreeNode* old, const int mode, const int child, const int used_old,
                                                   const int nl0, const double* __restrict__ reward, int& kept_n, int& kept_nodes) {
#pragma clang fp contract(off)
    const double ninf = -__builtin_inf();
    XrTreeRow* const rs = v.rs;
    XrTreeNode* const nodes = v.nodes;
    const int lane = v.lane;
    kept_n = 0; kept_nodes = 0;
    if (mode == 0) {
        if (lane == 0) xr_tree_init_row(v, nl0);
    } else if (mode == 1) {
        for (int i = lane; i < used_old; i += 64) nodes[i] = old[i];
        kept_n = old[0].N;
        kept_nodes = used_old;
        if (lane == 0) { rs->best = ninf; rs->max_depth = 0; rs->flags = XR_TREE_KEPT; }
    } else {
        const double r = *reward;
        kept_n = old[child].N;
        const int nused = xr_tree_keep_compact(old, nodes, child, used_old, v.node_cap, r, lane);
        kept_nodes = nused;
        if (lane == 0) {
            rs->mn = rs->mn - r; rs->mx = rs->mx - r; rs->best = ninf;
            rs->used = nused; rs->max_depth = 0; rs->flags = XR_TREE_KEPT;
        }
    }
    __syncthreads();
}

__global__ void __launch_bounds__(64) xr_tree_keep_begin_kernel(XrBatchDev src, XrTreeDev t, XrTreeKeepDev kp) {
#pragma clang fp contract(off)
    const int row = blockIdx.x, lane = threadIdx.x;
    const int e = t.env_lo + row;
    const int words = src.legal_words;
    // 1. the row's outputs
    xr_tree_clear_outputs(t.visits_out, t.value_out, t.best_order_out, t.info_out, t.best_return_out, row, t.k_cap, lane);
    XrTreeRow* const rs = t.rs + row;
    XrTreeNode* const nodes = t.nodes + (int64_t)row * t.node_cap;
    const XrTreeView v = {nodes, rs, t.node_cap, t.k_cap, words, lane};
    const XrTreeNode* const old = kp.old_nodes + (int64_t)row * t.node_cap;
    XrTreeKey* const key = kp.key + row;
    uint64_t* const klegal = kp.key_legal + (int64_t)row * words;
    const uint64_t* const legal = src.legal + (int64_t)e * words;
    const int nl0 = __builtin_amdgcn_readfirstlane(src.nlegal[e]);
    const int64_t steps = src.env_steps[e];
    const int region = src.env_region[e], replay = src.env_replay[e];
    // 2. the key: mode 0 rebuild, 1 the env has not moved (the whole tree), 2 the subtree below `child`
    int child, used_old;
    const int a = kp.played ? __builtin_amdgcn_readfirstlane(kp.played[row]) : -1;
    const int mode = xr_tree_keep_mode(old, rs, key, klegal, legal, words, a, nl0, steps, region, replay, t.node_cap, kp.n_add, lane, child, used_old);
    // 3. the tree
    int kept_n, kept_nodes;
    xr_tree_keep_build(v, old, mode, child, used_old, nl0, src.reward + e, kept_n, kept_nodes);
    // 4. an unexpanded root (a rebuilt row's, or a kept child no simulation has left yet) gets its children under this call's prior
    // (every lane; the block's next reader is the next kernel)
    if (nl0 > 0 && __builtin_amdgcn_readfirstlane(nodes[0].first) < 0)
        xr_tree_expand_block(v, 0, legal, nullptr, nl0, t.prior ? t.prior + (int64_t)row * t.k_cap : nullptr);
    // 5. the key of the state this tree belongs to
    for (int wd = lane; wd < words; wd += 64) klegal[wd] = legal[wd];
    if (lane == 0) {
        XrTreeKey k;
        k.env_steps = steps; k.region = region; k.replay = replay; k.valid = 1; k.pad = 0;
        *key = k;
        if (kp.kept_out) {
            kp.kept_out[(int64_t)row * 2] = kept_n;
            kp.kept_out[(int64_t)row * 2 + 1] = kept_nodes;
        }
    }
}
