// xr_tree.h — tree search (xr_batch_tree_search, "XR-Tree v1" of include/xroute_hip.h): pUCT over net orderings with the tree in device
// memory.  Included by xr_kernels.hip after xr_rollout.h; no router source changes.  One wavefront per row (an env of the caller), one
// tree per row in the row's pool of node_cap nodes; a search is n_waves x {select, xr_rollout_kernel, backup}, all in stream order.
//
//   xr_tree_reset_kernel    clears the row's outputs and its search state, makes the root and expands it
//   xr_tree_select_kernel   the n_par lanes of one wave descend one after the other: the 64 threads score the children of a node, a
//                           wave reduction takes the maximum (ties to the lowest net), the pending visits V of the finished lanes spread
//                           the later ones; each path is written as the prefix the rollout launch then plays
//   xr_tree_backup_kernel   simulations in lane order: N += 1, V -= 1, W += G along the path, min / max / best; after the last wave it
//                           writes the root's visit counts and values
// Every double operation of the spec is one IEEE operation: contraction is off in every function here, nothing calls log or sqrt (the
// exploration table comes from the host).  Thread 0 alone writes the tree; the other threads read it after a workgroup barrier (one wave:
// a fence and no wait).  The batch's own rows are only ever read, no workgroup waits for another one.
#pragma once

__device__ __forceinline__ double xr_tree_weight(const float* __restrict__ w, const int net, const int k_cap) {
    if (net > k_cap) return 0.0;
    const float x = w[net - 1];
    return (x >= 0.0f && x <= 3.4028234663852886e38f) ? (double)x : 0.0;      // not finite or < 0 counts as 0 (a NaN fails both tests)
}

// Thread 0: one child per legal net of `node` (the env's legal set minus the nets of the path, `mask`; null: the root), a contiguous block
// in ascending net order.  A block that does not fit leaves the node unexpanded and flags the row.
__device__ __forceinline__ void xr_tree_expand(const XrTreeDev& t, XrTreeNode* __restrict__ nodes, XrTreeRow* __restrict__ rs, const int node,
                                               const uint64_t* __restrict__ legal, const uint64_t* mask, const int words, const int cnt,
                                               const float* __restrict__ w) {
#pragma clang fp contract(off)
    const int first = rs->used;
    if (cnt > t.node_cap - first) {
        rs->flags |= XR_TREE_POOL_FULL;
        return;
    }
    rs->used = first + cnt;
    double S = 0.0;
    if (w)
        for (int wd = 0; wd < words; wd++) {
            uint64_t m = legal[wd] & (mask ? ~mask[wd] : ~0ull);
            while (m) {
                const int bit = __ffsll((long long)m) - 1;
                m &= m - 1;
                S += xr_tree_weight(w, wd * 64 + bit + 1, t.k_cap);
            }
        }
    const bool uniform = !w || !(S > 0.0);
    const double pu = 1.0 / (double)cnt;
    int c = 0;
    for (int wd = 0; wd < words && c < cnt; wd++) {
        uint64_t m = legal[wd] & (mask ? ~mask[wd] : ~0ull);
        while (m && c < cnt) {          // (c < cnt: the block is never overrun, whatever legal and nlegal say)
            const int bit = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int net = wd * 64 + bit + 1;
            XrTreeNode ch;
            ch.W = 0.0; ch.P = uniform ? pu : xr_tree_weight(w, net, t.k_cap) / S;
            ch.N = 0; ch.V = 0; ch.first = -1; ch.count = 0; ch.net = net; ch.pad = 0;
            nodes[first + c] = ch;
            c++;
        }
    }
    nodes[node].count = c;
    nodes[node].first = first;
}

__global__ void __launch_bounds__(64) xr_tree_reset_kernel(XrBatchDev src, XrTreeDev t) {
#pragma clang fp contract(off)
    const int row = blockIdx.x, lane = threadIdx.x;
    const int e = t.env_lo + row;
    const double ninf = -__builtin_inf();
    for (int k = lane; k < t.k_cap; k += 64) {
        t.visits_out[(int64_t)row * t.k_cap + k] = 0;
        t.value_out[(int64_t)row * t.k_cap + k] = ninf;
        if (t.best_order_out) t.best_order_out[(int64_t)row * t.k_cap + k] = 0;
    }
    if (lane != 0) return;
    int32_t* info = t.info_out + (int64_t)row * 4;
    info[0] = 0; info[1] = 0; info[2] = 0; info[3] = 0;
    if (t.best_return_out) t.best_return_out[row] = ninf;
    XrTreeRow* rs = t.rs + row;
    rs->mn = __builtin_inf(); rs->mx = ninf; rs->best = ninf;
    rs->used = 0; rs->max_depth = 0; rs->flags = 0; rs->pad = 0;
    const int nl0 = src.nlegal[e];
    if (nl0 <= 0) return;          // a done env: no tree, no simulation
    XrTreeNode* nodes = t.nodes + (int64_t)row * t.node_cap;
    XrTreeNode root;
    root.W = 0.0; root.P = 1.0; root.N = 0; root.V = 0; root.first = -1; root.count = 0; root.net = 0; root.pad = 0;
    nodes[0] = root;
    rs->used = 1;
    xr_tree_expand(t, nodes, rs, 0, src.legal + (int64_t)e * src.legal_words, nullptr, src.legal_words, nl0,
                   t.prior ? t.prior + (int64_t)row * t.k_cap : nullptr);
}

// dynamic LDS: uint64 [legal_words] nets of the path, int32 [k_cap + 1] nodes of the path, int32 [k_cap] nets of the path
__global__ void __launch_bounds__(64) xr_tree_select_kernel(XrBatchDev src, XrTreeDev t, int wave) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char tree_smem[];
    const int row = blockIdx.x, lane = threadIdx.x;
    const int e = t.env_lo + row;
    const int words = src.legal_words, k_cap = t.k_cap, n_par = t.n_par;
    uint64_t* const s_mask = reinterpret_cast<uint64_t*>(tree_smem);
    int32_t* const s_nodes = reinterpret_cast<int32_t*>(s_mask + words);
    int32_t* const s_nets = s_nodes + k_cap + 1;
    const int nl0 = __builtin_amdgcn_readfirstlane(src.nlegal[e]);
    int32_t* const pfx = t.prefix + (int64_t)row * n_par * k_cap;
    int32_t* const pout = t.paths_out ? t.paths_out + ((int64_t)row * t.n_sims + (int64_t)wave * n_par) * k_cap : nullptr;
    if (nl0 <= 0) {              // a done env: empty paths (the rollout launch answers them with the empty rollout)
        for (int64_t i = lane; i < (int64_t)n_par * k_cap; i += 64) {
            pfx[i] = 0;
            if (pout) pout[i] = 0;
        }
        return;
    }
    XrTreeNode* const nodes = t.nodes + (int64_t)row * t.node_cap;
    XrTreeRow* const rs = t.rs + row;
    const uint64_t* const legal = src.legal + (int64_t)e * words;
    const float* const w = t.prior ? t.prior + (int64_t)row * k_cap : nullptr;
    const double mn = rs->mn, mx = rs->mx;          // (backup alone changes them)
    const bool spread = mx > mn;
    const double span = mx - mn;
    for (int j = 0; j < n_par; j++) {
        for (int wd = lane; wd < words; wd += 64) s_mask[wd] = 0;
        __syncthreads();
        int node = 0, depth = 0;
        for (;;) {
            const int first = __builtin_amdgcn_readfirstlane(nodes[node].first);
            if (first < 0 || depth >= k_cap) break;
            const int cnt = __builtin_amdgcn_readfirstlane(nodes[node].count);
            const int n_p = __builtin_amdgcn_readfirstlane(nodes[node].N + nodes[node].V);
            const double Ep = t.E[n_p < t.e_max ? n_p : t.e_max];
            double bs = 0.0;
            int bi = 0x7FFFFFFF;
            for (int c = lane; c < cnt; c += 64) {
                const XrTreeNode ch = nodes[first + c];
                const int n_c = ch.N + ch.V;
                const double u = (Ep * ch.P) / (double)(n_c + 1);
                double v = 0.0;
                if (ch.N > 0 && spread) v = (ch.W / (double)ch.N - mn) / span;
                const double s = u + v;
                if (bi == 0x7FFFFFFF || s > bs) { bs = s; bi = c; }
            }
            for (int off = 32; off > 0; off >>= 1) {
                const double os = __shfl_xor(bs, off, 64);
                const int oi = __shfl_xor(bi, off, 64);
                if (oi != 0x7FFFFFFF && (bi == 0x7FFFFFFF || os > bs || (os == bs && oi < bi))) { bs = os; bi = oi; }
            }
            bi = __builtin_amdgcn_readfirstlane(bi);
            if (bi >= cnt) break;          // (an expanded node has children)
            const int child = first + bi;
            const int net = __builtin_amdgcn_readfirstlane(nodes[child].net);
            // every thread writes the same values: no divergent region inside the descent
            s_nets[depth] = net;
            s_nodes[depth + 1] = child;
            const int mw = (net - 1) >> 6;
            if (mw >= 0 && mw < words) s_mask[mw] = s_mask[mw] | (1ull << ((net - 1) & 63));
            depth++;
            node = child;
        }
        __syncthreads();
        if (lane == 0) {
            if (depth < nl0 && nodes[node].first < 0) xr_tree_expand(t, nodes, rs, node, legal, s_mask, words, nl0 - depth, w);
            nodes[0].V += 1;
            for (int d = 1; d <= depth; d++) nodes[s_nodes[d]].V += 1;
            if (depth > rs->max_depth) rs->max_depth = depth;
        }
        for (int k = lane; k < k_cap; k += 64) {
            const int net = k < depth ? s_nets[k] : 0;
            pfx[(int64_t)j * k_cap + k] = net;
            if (pout) pout[(int64_t)j * k_cap + k] = net;
        }
        __syncthreads();          // thread 0's nodes and counts, before the next lane reads them
    }
}

__global__ void __launch_bounds__(64) xr_tree_backup_kernel(XrBatchDev src, XrTreeDev t, int wave, int last) {
#pragma clang fp contract(off)
    const int row = blockIdx.x, lane = threadIdx.x;
    const int e = t.env_lo + row;
    const int k_cap = t.k_cap, n_par = t.n_par;
    if (__builtin_amdgcn_readfirstlane(src.nlegal[e]) <= 0) {
        if (t.returns_out && lane == 0)
            for (int j = 0; j < n_par; j++) t.returns_out[(int64_t)row * t.n_sims + (int64_t)wave * n_par + j] = t.ret[(int64_t)row * n_par + j];
        return;
    }
    XrTreeNode* const nodes = t.nodes + (int64_t)row * t.node_cap;
    XrTreeRow* const rs = t.rs + row;
    double mn = rs->mn, mx = rs->mx, best = rs->best;
    for (int j = 0; j < n_par; j++) {
        const double G = t.ret[(int64_t)row * n_par + j];
        const int32_t* const pfx = t.prefix + ((int64_t)row * n_par + j) * k_cap;
        int node = 0;
        for (int d = 0;; d++) {
            if (lane == 0) {
                XrTreeNode* p = nodes + node;
                p->N += 1; p->V -= 1; p->W += G;
            }
            if (d >= k_cap) break;
            const int net = __builtin_amdgcn_readfirstlane(pfx[d]);
            if (net <= 0) break;
            const int first = __builtin_amdgcn_readfirstlane(nodes[node].first);
            const int cnt = __builtin_amdgcn_readfirstlane(nodes[node].count);
            if (first < 0) break;
            int found = 0x7FFFFFFF;
            for (int c = lane; c < cnt; c += 64)
                if (nodes[first + c].net == net && c < found) found = c;
            for (int off = 32; off > 0; off >>= 1) {
                const int o = __shfl_xor(found, off, 64);
                found = o < found ? o : found;
            }
            found = __builtin_amdgcn_readfirstlane(found);
            if (found >= cnt) break;          // (select wrote the path from these very children)
            node = first + found;
        }
        mn = fmin(mn, G);
        mx = fmax(mx, G);
        if (G > best) {
            best = G;
            if (t.best_order_out)
                for (int k = lane; k < k_cap; k += 64) t.best_order_out[(int64_t)row * k_cap + k] = t.order[((int64_t)row * n_par + j) * k_cap + k];
        }
        if (t.returns_out && lane == 0) t.returns_out[(int64_t)row * t.n_sims + (int64_t)wave * n_par + j] = G;
    }
    if (lane == 0) { rs->mn = mn; rs->mx = mx; rs->best = best; }
    if (!last) return;
    __syncthreads();          // thread 0's counts and sums, before every thread reads the root's children
    const int first = __builtin_amdgcn_readfirstlane(nodes[0].first);
    const int cnt = __builtin_amdgcn_readfirstlane(nodes[0].count);
    if (first >= 0)
        for (int c = lane; c < cnt; c += 64) {
            const XrTreeNode ch = nodes[first + c];
            if (ch.net < 1 || ch.net > k_cap) continue;
            t.visits_out[(int64_t)row * k_cap + ch.net - 1] = ch.N;
            if (ch.N > 0) t.value_out[(int64_t)row * k_cap + ch.net - 1] = ch.W / (double)ch.N;
        }
    if (lane == 0) {
        int32_t* info = t.info_out + (int64_t)row * 4;
        info[0] = (wave + 1) * n_par; info[1] = rs->used; info[2] = rs->max_depth; info[3] = rs->flags;
        if (t.best_return_out) t.best_return_out[row] = best;
    }
}
