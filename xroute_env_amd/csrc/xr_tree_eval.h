// xr_tree_eval.h — evaluated tree search (xr_batch_tree_open / _leaves / _backup, "XR-Tree v2, evaluated" of include/xroute_hip.h): pUCT
// whose simulations stop at the selected leaf; the caller's evaluator values the leaf's state and may give a prior for its children.
// Included by xr_kernels.hip after xr_tree_keep.h; the node, the row state and xr_tree_weight are xr_tree.h's.  One wavefront per row.
//
//   xr_tree_eval_open_kernel     copies the env's nlegal and legal words (and the row's prior) into the pool — every later kernel of the
//                                session reads the copy, never the env — resets the row state, makes the root and expands it
//   xr_tree_eval_select_kernel   v1's descent for the n_par lanes of a wave, one after the other; a fresh leaf is expanded here under the
//                                open call's row prior; writes the paths (the prefix of the peek launch) and the leaf records
//   xr_tree_eval_backup_kernel   simulations in lane order: G = the line's return (+ the evaluator's value unless the leaf is terminal),
//                                N += 1, V -= 1, W += G along the path, min / max, the best terminal line; then the evaluator's prior
//                                over the children of a fresh leaf; then the root's visit counts and values
// Every double operation of the spec is one IEEE operation: contraction is off in every function here, nothing calls log or sqrt.  Thread
// 0 alone writes the fields of existing nodes and the row state; a new children block and the P of a block are written by the 64 lanes,
// one child each (64 at a time), and read by the others after a workgroup barrier (one wave: a fence and no wait).  No workgroup waits
// for another one.
#pragma once

// All 64 lanes: one child per net of (legal & ~mask) for `node`, a contiguous block in ascending net order: v1's expansion and v1's Prior
// rule, the block written 64 children at a time (lane b takes bit b of a legal word).  1: the block was made; 0: it does not fit (the
// row is flagged).  The caller puts a barrier before the block is read.
__device__ __forceinline__ int xr_tree_eval_expand(const XrTreeEvalDev& t, XrTreeNode* __restrict__ nodes, XrTreeRow* __restrict__ rs, const int node,
                                                   const uint64_t* __restrict__ legal, const uint64_t* mask, const int cnt, const float* __restrict__ w,
                                                   const int lane) {
#pragma clang fp contract(off)
    const int words = t.legal_words;
    const int first = __builtin_amdgcn_readfirstlane(rs->used);
    if (cnt < 1 || first < 1 || cnt > t.node_cap - first) {
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
                S += xr_tree_weight(w, wd * 64 + bit + 1, t.k_cap);
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
                XrTreeNode ch;
                ch.W = 0.0; ch.P = uniform ? pu : xr_tree_weight(w, net, t.k_cap) / S;
                ch.N = 0; ch.V = 0; ch.first = -1; ch.count = 0; ch.net = net; ch.pad = 0;
                nodes[first + c] = ch;
            }
        }
        base += __popcll(m);
    }
    if (base < cnt)          // (never: nlegal counts the bits of the legal words) — the children past the bits are never read
        for (int c = base + lane; c < cnt; c += 64) {
            XrTreeNode ch;
            ch.W = 0.0; ch.P = 0.0; ch.N = 0; ch.V = 0; ch.first = -1; ch.count = 0; ch.net = 0; ch.pad = 0;
            nodes[first + c] = ch;
        }
    if (lane == 0) {
        rs->used = first + cnt;
        nodes[node].count = base < cnt ? base : cnt;
        nodes[node].first = first;
    }
    return 1;
}

__global__ void __launch_bounds__(64) xr_tree_eval_open_kernel(XrBatchDev src, XrTreeEvalDev t, const float* __restrict__ root_prior) {
#pragma clang fp contract(off)
    const int row = blockIdx.x, lane = threadIdx.x;
    const int e = t.env_lo + row;
    const int words = t.legal_words, k_cap = t.k_cap;
    const double ninf = -__builtin_inf();
    uint64_t* const legal = t.legal + (int64_t)row * words;
    for (int wd = lane; wd < words; wd += 64) legal[wd] = src.legal[(int64_t)e * words + wd];
    for (int k = lane; k < k_cap; k += 64) {
        t.best_order[(int64_t)row * k_cap + k] = 0;
        t.prior[(int64_t)row * k_cap + k] = root_prior ? root_prior[(int64_t)row * k_cap + k] : 0.0f;
    }
    int nl0 = __builtin_amdgcn_readfirstlane(src.nlegal[e]);
    if (nl0 > k_cap) nl0 = k_cap;          // (never: nlegal <= k_max <= k_cap)
    XrTreeRow* const rs = t.rs + row;
    XrTreeNode* const nodes = t.nodes + (int64_t)row * t.node_cap;
    if (lane == 0) {
        t.nlegal[row] = nl0;
        rs->mn = __builtin_inf(); rs->mx = ninf; rs->best = ninf;
        rs->used = 0; rs->max_depth = 0; rs->flags = 0; rs->pad = 0;
        if (nl0 > 0) {
            XrTreeNode root;
            root.W = 0.0; root.P = 1.0; root.N = 0; root.V = 0; root.first = -1; root.count = 0; root.net = 0; root.pad = 0;
            nodes[0] = root;
            rs->used = 1;
        }
    }
    __syncthreads();          // the copies and the root, before every lane reads them
    if (nl0 <= 0) return;          // a done env: no tree, no simulation
    xr_tree_eval_expand(t, nodes, rs, 0, legal, nullptr, nl0, t.has_prior ? t.prior + (int64_t)row * k_cap : nullptr, lane);
}

// dynamic LDS: uint64 [legal_words] nets of the path, int32 [k_cap + 1] nodes of the path, int32 [k_cap] nets of the path
__global__ void __launch_bounds__(64) xr_tree_eval_select_kernel(XrTreeEvalDev t, int32_t* __restrict__ paths_out, int32_t* __restrict__ leaf_out) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char tree_eval_smem[];
    const int row = blockIdx.x, lane = threadIdx.x;
    const int words = t.legal_words, k_cap = t.k_cap, n_par = t.n_par;
    uint64_t* const s_mask = reinterpret_cast<uint64_t*>(tree_eval_smem);
    int32_t* const s_nodes = reinterpret_cast<int32_t*>(s_mask + words);
    int32_t* const s_nets = s_nodes + k_cap + 1;
    const int nl0 = __builtin_amdgcn_readfirstlane(t.nlegal[row]);
    int32_t* const pfx = t.prefix + (int64_t)row * n_par * k_cap;
    int32_t* const pout = paths_out ? paths_out + (int64_t)row * n_par * k_cap : nullptr;
    int32_t* const leaf = t.leaf + (int64_t)row * n_par * 2;
    int32_t* const lout = leaf_out ? leaf_out + (int64_t)row * n_par * 2 : nullptr;
    if (nl0 <= 0) {              // a done row: empty paths (the peek launch answers them with the env's current state), no leaf
        for (int64_t i = lane; i < (int64_t)n_par * k_cap; i += 64) {
            pfx[i] = 0;
            if (pout) pout[i] = 0;
        }
        for (int i = lane; i < n_par * 2; i += 64) {
            const int v = (i & 1) ? XR_TREE_LEAF_NONE : -1;
            leaf[i] = v;
            if (lout) lout[i] = v;
        }
        return;
    }
    XrTreeNode* const nodes = t.nodes + (int64_t)row * t.node_cap;
    XrTreeRow* const rs = t.rs + row;
    const uint64_t* const legal = t.legal + (int64_t)row * words;
    const float* const w = t.has_prior ? t.prior + (int64_t)row * k_cap : nullptr;
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
            if (first > t.node_cap - cnt) break;          // (never: expand hands out blocks inside the pool)
            const int n_p = __builtin_amdgcn_readfirstlane(nodes[node].N + nodes[node].V);
            const double Ep = t.E[n_p < 0 ? 0 : (n_p < t.e_max ? n_p : t.e_max)];
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
            if (net >= 1 && mw < words) s_mask[mw] = s_mask[mw] | (1ull << ((net - 1) & 63));
            depth++;
            node = child;
        }
        __syncthreads();
        int flags = 0;
        if (depth >= nl0) flags = XR_TREE_LEAF_TERMINAL;
        else if (__builtin_amdgcn_readfirstlane(nodes[node].first) < 0 && xr_tree_eval_expand(t, nodes, rs, node, legal, s_mask, nl0 - depth, w, lane))
            flags = XR_TREE_LEAF_FRESH;
        __syncthreads();          // the block, before thread 0 goes on and the next lane descends into it
        if (lane == 0) {
            nodes[0].V += 1;
            for (int d = 1; d <= depth; d++) nodes[s_nodes[d]].V += 1;
            if (depth > rs->max_depth) rs->max_depth = depth;
            leaf[j * 2] = node; leaf[j * 2 + 1] = flags;
            if (lout) { lout[j * 2] = node; lout[j * 2 + 1] = flags; }
        }
        for (int k = lane; k < k_cap; k += 64) {
            const int net = k < depth ? s_nets[k] : 0;
            pfx[(int64_t)j * k_cap + k] = net;
            if (pout) pout[(int64_t)j * k_cap + k] = net;
        }
        __syncthreads();          // thread 0's counts, before the next lane reads them
    }
}

__global__ void __launch_bounds__(64) xr_tree_eval_backup_kernel(XrTreeEvalDev t, const double* __restrict__ value, const float* __restrict__ leaf_prior,
                                                                 int sims, int32_t* __restrict__ visits_out, double* __restrict__ value_out,
                                                                 int32_t* __restrict__ info_out, int32_t* __restrict__ best_order_out,
                                                                 double* __restrict__ best_return_out, double* __restrict__ returns_out) {
#pragma clang fp contract(off)
    const int row = blockIdx.x, lane = threadIdx.x;
    const int k_cap = t.k_cap, n_par = t.n_par;
    const double ninf = -__builtin_inf();
    for (int k = lane; k < k_cap; k += 64) {
        visits_out[(int64_t)row * k_cap + k] = 0;
        value_out[(int64_t)row * k_cap + k] = ninf;
    }
    int32_t* const info = info_out + (int64_t)row * 4;
    if (__builtin_amdgcn_readfirstlane(t.nlegal[row]) <= 0) {          // a done row: v1's empty result
        if (best_order_out)
            for (int k = lane; k < k_cap; k += 64) best_order_out[(int64_t)row * k_cap + k] = 0;
        if (returns_out)
            for (int j = lane; j < n_par; j += 64) returns_out[(int64_t)row * n_par + j] = 0.0;
        if (lane == 0) {
            info[0] = 0; info[1] = 0; info[2] = 0; info[3] = 0;
            if (best_return_out) best_return_out[row] = ninf;
        }
        return;
    }
    XrTreeNode* const nodes = t.nodes + (int64_t)row * t.node_cap;
    XrTreeRow* const rs = t.rs + row;
    int32_t* const best_order = t.best_order + (int64_t)row * k_cap;
    const int used = __builtin_amdgcn_readfirstlane(rs->used);          // (backup makes no node)
    double mn = rs->mn, mx = rs->mx, best = rs->best;
    for (int j = 0; j < n_par; j++) {
        const int leaf_node = __builtin_amdgcn_readfirstlane(t.leaf[((int64_t)row * n_par + j) * 2]);
        const int flags = __builtin_amdgcn_readfirstlane(t.leaf[((int64_t)row * n_par + j) * 2 + 1]);
        const double ret = t.ret[(int64_t)row * n_par + j];
        double G = ret;
        if (!(flags & XR_TREE_LEAF_TERMINAL)) {
            double v = value[(int64_t)row * n_par + j];
            if (!(v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308)) v = 0.0;          // not finite counts as 0 (a NaN fails both tests)
            G = ret + v;
        }
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
            if (first < 0 || first > used - cnt) break;
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
        if ((flags & XR_TREE_LEAF_TERMINAL) && G > best) {          // only a terminal line's G is an episode return
            best = G;
            for (int k = lane; k < k_cap; k += 64) best_order[k] = pfx[k];
        }
        if (returns_out && lane == 0) returns_out[(int64_t)row * n_par + j] = G;
        // the evaluator's prior over the children of the leaf this lane expanded: v1's Prior rule on that lane's row
        if (leaf_prior && (flags & XR_TREE_LEAF_FRESH) && leaf_node >= 0 && leaf_node < used) {
            const int first = __builtin_amdgcn_readfirstlane(nodes[leaf_node].first);
            const int cnt = __builtin_amdgcn_readfirstlane(nodes[leaf_node].count);
            if (first >= 1 && cnt >= 1 && first <= used - cnt) {
                const float* const w = leaf_prior + ((int64_t)row * n_par + j) * k_cap;
                double S = 0.0;          // every lane adds the same numbers in the same (ascending net) order
                for (int c = 0; c < cnt; c++) {
                    const int net = nodes[first + c].net;
                    if (net >= 1) S += xr_tree_weight(w, net, k_cap);
                }
                if (S > 0.0)
                    for (int c = lane; c < cnt; c += 64) {
                        const int net = nodes[first + c].net;
                        nodes[first + c].P = net >= 1 ? xr_tree_weight(w, net, k_cap) / S : 0.0;
                    }
            }
        }
        __syncthreads();          // thread 0's sums and the block's P, before the next lane's walk
    }
    if (lane == 0) { rs->mn = mn; rs->mx = mx; rs->best = best; }
    __syncthreads();          // thread 0's counts and sums, before every thread reads the root's children
    const int first = __builtin_amdgcn_readfirstlane(nodes[0].first);
    const int cnt = __builtin_amdgcn_readfirstlane(nodes[0].count);
    if (first >= 1 && first <= used - cnt)
        for (int c = lane; c < cnt; c += 64) {
            const XrTreeNode ch = nodes[first + c];
            if (ch.net < 1 || ch.net > k_cap) continue;
            visits_out[(int64_t)row * k_cap + ch.net - 1] = ch.N;
            if (ch.N > 0) value_out[(int64_t)row * k_cap + ch.net - 1] = ch.W / (double)ch.N;
        }
    if (best_order_out)
        for (int k = lane; k < k_cap; k += 64) best_order_out[(int64_t)row * k_cap + k] = best_order[k];
    if (lane == 0) {
        info[0] = sims; info[1] = rs->used; info[2] = rs->max_depth; info[3] = rs->flags;
        if (best_return_out) best_return_out[row] = best;
    }
}
