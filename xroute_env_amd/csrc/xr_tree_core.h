// xr_tree_core.h — the pUCT tree of "XR-Tree v1" (include/xroute_hip.h; the executable spec is tests/tree_twin.py's RowTree), each rule
// once.  Included by xr_kernels.hip before xr_tree.h; the plain (xr_tree.h), kept (xr_tree_keep.h) and evaluated (xr_tree_eval.h)
// searches are kernels around these functions, as the kept and evaluated twins are subclasses of RowTree.  One wavefront per row.
//
//   xr_tree_init_row, xr_tree_clear_outputs   an empty search: the row state and the unexpanded root; the row's outputs
//   xr_tree_expand_block                      one child per legal net of a node, a contiguous block in ascending net order, the Prior rule
//   xr_tree_descend, xr_tree_finish_lane      Select for one lane of a wave: the descent by score, then V += 1 and the prefix written out
//   xr_tree_child_by_net                      the child of a block that carries a net
//   xr_tree_backup_sim, xr_tree_write_root    Backup for one simulation; the root's visit counts and values and the info row
// Every double operation of the spec is one IEEE operation: contraction is off in every function here, nothing calls log or sqrt (the
// exploration table comes from the host), ties go to the lowest child.  Thread 0 alone writes the fields of existing nodes and the row
// state; a new children block is written by the 64 lanes, one child each (64 at a time), and read by the others after a workgroup
// barrier (one wave: a fence and no wait).  The guards marked (never) hold on every tree these functions build; they keep a damaged
// pool from sending an index out of it.  No workgroup waits for another one.
#pragma once

// One row's tree as the rules see it, built inside a kernel from XrTreeDev or XrTreeEvalDev.
struct XrTreeView {
    XrTreeNode* nodes;          // the row's pool, node_cap nodes; node 0 is the root
    XrTreeRow* rs;
    int node_cap, k_cap, words, lane;
};

// The path of the descending lane, in dynamic LDS: uint64 [words] nets of the path, int32 [k_cap + 1] nodes of the path, int32 [k_cap] nets
// of the path (the size the two select launchers ask for).
struct XrTreePath {
    uint64_t* mask;
    int32_t* nodes;
    int32_t* nets;
};

__device__ __forceinline__ XrTreePath xr_tree_path(char* smem, const int words, const int k_cap) {
    XrTreePath p;
    p.mask = reinterpret_cast<uint64_t*>(smem);
    p.nodes = reinterpret_cast<int32_t*>(p.mask + words);
    p.nets = p.nodes + k_cap + 1;
    return p;
}

__device__ __forceinline__ double xr_tree_weight(const float* __restrict__ w, const int net, const int k_cap) {
    if (net > k_cap) return 0.0;
    const float x = w[net - 1];
    return (x >= 0.0f && x <= 3.4028234663852886e38f) ? (double)x : 0.0;      // not finite or < 0 counts as 0 (a NaN fails both tests)
}

// an unvisited, unexpanded node
__device__ __forceinline__ XrTreeNode xr_tree_new_node(const double P, const int net) {
    XrTreeNode nd;
    nd.W = 0.0; nd.P = P; nd.N = 0; nd.V = 0; nd.first = -1; nd.count = 0; nd.net = net; nd.pad = 0;
    return nd;
}

// Thread 0: the row state of an empty search and, for a live row (nl0 > 0), the unexpanded root.
__device__ __forceinline__ void xr_tree_init_row(const XrTreeView& v, const int nl0) {
#pragma clang fp contract(off)
    XrTreeRow* const rs = v.rs;
    rs->mn = __builtin_inf(); rs->mx = -__builtin_inf(); rs->best = -__builtin_inf();
    rs->used = 0; rs->max_depth = 0; rs->flags = 0; rs->pad = 0;
    if (nl0 <= 0) return;
    v.nodes[0] = xr_tree_new_node(1.0, 0);
    rs->used = 1;
}

// All 64 lanes: the row's outputs as a search without a simulation leaves them (best_order_out, best_return_out: null or given).
__device__ __forceinline__ void xr_tree_clear_outputs(int32_t* __restrict__ visits_out, double* __restrict__ value_out, int32_t* __restrict__ best_order_out,
                                                      int32_t* __restrict__ info_out, double* __restrict__ best_return_out, const int row, const int k_cap,
                                                      const int lane) {
#pragma clang fp contract(off)
    const double ninf = -__builtin_inf();
    for (int k = lane; k < k_cap; k += 64) {
        visits_out[(int64_t)row * k_cap + k] = 0;
        value_out[(int64_t)row * k_cap + k] = ninf;
        if (best_order_out) best_order_out[(int64_t)row * k_cap + k] = 0;
    }
    if (lane != 0) return;
    int32_t* const info = info_out + (int64_t)row * 4;
    info[0] = 0; info[1] = 0; info[2] = 0; info[3] = 0;
    if (best_return_out) best_return_out[row] = ninf;
}

// All 64 lanes: one child per net of (legal & ~mask) for `node` (mask: the nets of the path; null: the root), a contiguous block in
// ascending net order, written 64 children at a time (lane b takes bit b of a legal word; its child index is the popcount below it).
// Prior rule: P = w / S, S summed over the block's nets in ascending order; uniform without w or with S == 0.  1: the block was made;
// 0: it does not fit, the node stays unexpanded and the row is flagged.  The caller puts a barrier before the block is read.
__device__ __forceinline__ int xr_tree_expand_block(const XrTreeView& v, const int node, const uint64_t* __restrict__ legal, const uint64_t* mask,
                                                    const int cnt, const float* __restrict__ w) {
#pragma clang fp contract(off)
    XrTreeNode* const __restrict__ nodes = v.nodes;
    XrTreeRow* const __restrict__ rs = v.rs;
    const int words = v.words, lane = v.lane;
    const int first = __builtin_amdgcn_readfirstlane(rs->used);
    if (cnt < 1 || first < 1 || cnt > v.node_cap - first) {
        if (lane == 0) rs->flags |= XR_TREE_POOL_FULL;
        return 0;
    }
    double S = 0.0;          // every lane adds the same numbers in the same (ascending net) order
    if (w)
        for (int wd = 0; wd < words; wd++) {
            uint64_t m = legal[wd] & (mask ? ~mask[wd] : ~0ull);
            while (m) {
                const int bit = __ffsll((long long)m) - 1;
                m &= m - 1;
                S += xr_tree_weight(w, wd * 64 + bit + 1, v.k_cap);
            }
        }
    const bool uniform = !w || !(S > 0.0);
    const double pu = 1.0 / (double)cnt;
    int base = 0;
    for (int wd = 0; wd < words; wd++) {
        const uint64_t m = legal[wd] & (mask ? ~mask[wd] : ~0ull);
        if ((m >> lane) & 1ull) {
            const int c = base + __popcll(m & ((1ull << lane) - 1ull));
            if (c < cnt) {          // (the block is never overrun, whatever the legal words and nlegal say)
                const int net = wd * 64 + lane + 1;
                nodes[first + c] = xr_tree_new_node(uniform ? pu : xr_tree_weight(w, net, v.k_cap) / S, net);
            }
        }
        base += __popcll(m);
    }
    if (base < cnt)          // (never: nlegal counts the bits of the legal words) — the children past the bits are never read
        for (int c = base + lane; c < cnt; c += 64) nodes[first + c] = xr_tree_new_node(0.0, 0);
    if (lane == 0) {
        rs->used = first + cnt;
        nodes[node].count = base < cnt ? base : cnt;
        nodes[node].first = first;
    }
    return 1;
}

// All 64 lanes: the child of the block with the highest score = (Ep * P) / (n + 1) + ((N > 0 and max > min) ? (W / N - min) / (max - min) : 0),
// n = N + V; the maximum under `>`, ties to the lowest child.  The same value in every lane; >= cnt for an empty block.
__device__ __forceinline__ int xr_tree_best_child(const XrTreeNode* nodes, const int first, const int cnt, const double Ep, const double mn,
                                                  const double mx, const int lane) {
#pragma clang fp contract(off)
    const bool spread = mx > mn;
    const double span = mx - mn;
    double bs = 0.0;
    int bi = 0x7FFFFFFF;
    for (int c = lane; c < cnt; c += 64) {
        const XrTreeNode ch = nodes[first + c];
        const int n_c = ch.N + ch.V;
        const double u = (Ep * ch.P) / (double)(n_c + 1);
        double q = 0.0;
        if (ch.N > 0 && spread) q = (ch.W / (double)ch.N - mn) / span;
        const double s = u + q;
        if (bi == 0x7FFFFFFF || s > bs) { bs = s; bi = c; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double os = __shfl_xor(bs, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (oi != 0x7FFFFFFF && (bi == 0x7FFFFFFF || os > bs || (os == bs && oi < bi))) { bs = os; bi = oi; }
    }
    return __builtin_amdgcn_readfirstlane(bi);
}

// All 64 lanes, one lane of a wave: clears the path, descends from the root by xr_tree_best_child to an unexpanded or terminal node
// and records the path's nets, nodes and net mask in LDS.  Returns the node; depth: the length of the path.  mn, mx: the row's, as
// the last backup left them.  Both ends are workgroup barriers: the path is complete and readable by every thread on return.
__device__ __forceinline__ int xr_tree_descend(const XrTreeView& v, const double* __restrict__ E, const int e_max, const double mn, const double mx,
                                               const XrTreePath& p, int& depth_out) {
#pragma clang fp contract(off)
    const XrTreeNode* const nodes = v.nodes;
    for (int wd = v.lane; wd < v.words; wd += 64) p.mask[wd] = 0;
    __syncthreads();
    int node = 0, depth = 0;
    for (;;) {
        const int first = __builtin_amdgcn_readfirstlane(nodes[node].first);
        if (first < 0 || depth >= v.k_cap) break;
        const int cnt = __builtin_amdgcn_readfirstlane(nodes[node].count);
        if (first > v.node_cap - cnt) break;          // (never: expand hands out blocks inside the pool)
        const int n_p = __builtin_amdgcn_readfirstlane(nodes[node].N + nodes[node].V);
        const double Ep = E[n_p < 0 ? 0 : (n_p < e_max ? n_p : e_max)];
        const int bi = xr_tree_best_child(nodes, first, cnt, Ep, mn, mx, v.lane);
        if (bi >= cnt) break;          // (an expanded node has children)
        const int child = first + bi;
        const int net = __builtin_amdgcn_readfirstlane(nodes[child].net);
        // every thread writes the same values: no divergent region inside the descent
        p.nets[depth] = net;
        p.nodes[depth + 1] = child;
        const int mw = (net - 1) >> 6;
        if (net >= 1 && mw < v.words) p.mask[mw] = p.mask[mw] | (1ull << ((net - 1) & 63));
        depth++;
        node = child;
    }
    __syncthreads();
    depth_out = depth;
    return node;
}

// All 64 lanes, after the leaf decision of a lane: the pending visits V += 1 along its path — what spreads the later lanes of the wave —
// and the path as row j of the wave's prefixes (pout: null, or the caller's copy).  Starts and ends with a workgroup barrier: a block the leaf decision
// made, thread 0's counts and the row state, before the next lane descends.
__device__ __forceinline__ void xr_tree_finish_lane(const XrTreeView& v, const XrTreePath& p, const int depth, int32_t* __restrict__ pfx,
                                                    int32_t* __restrict__ pout, const int j) {
#pragma clang fp contract(off)
    __syncthreads();
    if (v.lane == 0) {
        v.nodes[0].V += 1;
        for (int d = 1; d <= depth; d++) v.nodes[p.nodes[d]].V += 1;
        if (depth > v.rs->max_depth) v.rs->max_depth = depth;
    }
    for (int k = v.lane; k < v.k_cap; k += 64) {
        const int net = k < depth ? p.nets[k] : 0;
        pfx[(int64_t)j * v.k_cap + k] = net;
        if (pout) pout[(int64_t)j * v.k_cap + k] = net;
    }
    __syncthreads();
}

// All 64 lanes, a done row: n empty prefix entries (the line launch answers an empty path without routing).
__device__ __forceinline__ void xr_tree_empty_prefixes(int32_t* __restrict__ pfx, int32_t* __restrict__ pout, const int64_t n, const int lane) {
    for (int64_t i = lane; i < n; i += 64) {
        pfx[i] = 0;
        if (pout) pout[i] = 0;
    }
}

// All 64 lanes: the index in its block of the child that carries `net` (the lowest, were there two); >= cnt: none.  The same value in
// every lane.
__device__ __forceinline__ int xr_tree_child_by_net(const XrTreeNode* nodes, const int first, const int cnt, const int net, const int lane) {
#pragma clang fp contract(off)
    int found = 0x7FFFFFFF;
    for (int c = lane; c < cnt; c += 64)
        if (nodes[first + c].net == net && c < found) found = c;
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(found, off, 64);
        found = o < found ? o : found;
    }
    return __builtin_amdgcn_readfirstlane(found);
}

// All 64 lanes, one simulation with return G and path pfx: N += 1, V -= 1, W += G at the root and along the path (thread 0 writes),
// then the row's min / max.  used: the row's nodes_used (backup makes no node).
__device__ __forceinline__ void xr_tree_backup_sim(const XrTreeView& v, const int used, const int32_t* __restrict__ pfx, const double G, double& mn,
                                                   double& mx) {
#pragma clang fp contract(off)
    XrTreeNode* const nodes = v.nodes;
    int node = 0;
    for (int d = 0;; d++) {
        if (v.lane == 0) {
            XrTreeNode* p = nodes + node;
            p->N += 1; p->V -= 1; p->W += G;
        }
        if (d >= v.k_cap) break;
        const int net = __builtin_amdgcn_readfirstlane(pfx[d]);
        if (net <= 0) break;
        const int first = __builtin_amdgcn_readfirstlane(nodes[node].first);
        const int cnt = __builtin_amdgcn_readfirstlane(nodes[node].count);
        if (first < 0 || first > used - cnt) break;
        const int found = xr_tree_child_by_net(nodes, first, cnt, net, v.lane);
        if (found >= cnt) break;          // (select wrote the path from these very children)
        node = first + found;
    }
    mn = fmin(mn, G);
    mx = fmax(mx, G);
}

// All 64 lanes, after the last backup_sim of a launch: the root's children into visits_out / value_out (cleared before), the info row
// {sims, nodes_used, max_depth, flags} and the best return.  Starts with a workgroup barrier: thread 0's counts and sums, before
// every thread reads the root's children.
__device__ __forceinline__ void xr_tree_write_root(const XrTreeView& v, const int used, int32_t* __restrict__ visits_out, double* __restrict__ value_out,
                                                   int32_t* __restrict__ info_out, double* __restrict__ best_return_out, const int row, const int sims,
                                                   const double best) {
#pragma clang fp contract(off)
    __syncthreads();
    const XrTreeNode* const nodes = v.nodes;
    const int k_cap = v.k_cap;
    const int first = __builtin_amdgcn_readfirstlane(nodes[0].first);
    const int cnt = __builtin_amdgcn_readfirstlane(nodes[0].count);
    if (first >= 1 && first <= used - cnt)
        for (int c = v.lane; c < cnt; c += 64) {
            const XrTreeNode ch = nodes[first + c];
            if (ch.net < 1 || ch.net > k_cap) continue;
            visits_out[(int64_t)row * k_cap + ch.net - 1] = ch.N;
            if (ch.N > 0) value_out[(int64_t)row * k_cap + ch.net - 1] = ch.W / (double)ch.N;
        }
    if (v.lane == 0) {
        int32_t* const info = info_out + (int64_t)row * 4;
        info[0] = sims; info[1] = v.rs->used; info[2] = v.rs->max_depth; info[3] = v.rs->flags;
        if (best_return_out) best_return_out[row] = best;
    }
}
