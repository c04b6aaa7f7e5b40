// xr_tree_eval.h — evaluated tree search (xr_batch_tree_open / _leaves / _backup, "XR-Tree v2, evaluated" of include/xroute_hip.h): pUCT
// whose simulations stop at the selected leaf; the caller's evaluator values the leaf's state and may give a prior for its children.
// Included by xr_kernels.hip after xr_tree_keep.h.  One wavefront per row.  The tree's rules — expansion, the descent, the backup of a
// simulation, the root's results — are xr_tree_core.h's, the very functions the plain search runs; what is this form's own: the pool's
// snapshot of the env's nlegal and legal words, the leaf records, how G is formed, which lines may become the best one, the
// evaluator's prior over a fresh leaf's children, and outputs written after every wave.
//
//   xr_tree_eval_open_kernel     copies the env's nlegal and legal words (and the row's prior) into the pool — every later kernel of the
//                                session reads the copy, never the env — resets the row state, makes the root and expands it
//   xr_tree_eval_reopen_kernel   the same for a session that continues ("XR-Tree v2, kept"): checks the row's key, re-roots the last
//                                session's tree below the played net into the pool's other half (xr_tree_keep.h's functions), keeps it
//                                whole, or rebuilds the row as the open kernel does; then the snapshot, the row prior and the new key
//   xr_tree_eval_select_kernel   the descent for the n_par lanes of a wave, one after the other; a fresh leaf is expanded here under the
//                                open call's row prior; writes the paths (the prefix of the peek launch) and the leaf records
//   xr_tree_eval_backup_kernel   simulations in lane order: G = the line's return (+ the evaluator's value unless the leaf is terminal),
//                                the backup of G, the best terminal line; then the evaluator's prior over the children of a fresh leaf;
//                                then the root's visit counts and values
// Contraction is off in every function.  Thread 0 alone writes the fields of existing nodes and the row state; a new children block and
// the P of a block are written by the 64 lanes, one child each (64 at a time), and read by the others after a workgroup barrier (one
// wave: a fence and no wait).  No workgroup waits for another one.
#pragma once

__global__ void __launch_bounds__(64) xr_tree_eval_open_kernel(XrBatchDev src, XrTreeEvalDev t, const float* __restrict__ root_prior) {
#pragma clang fp contract(off)
    const int row = blockIdx.x, lane = threadIdx.x;
    const int e = t.env_lo + row;
    const int words = t.legal_words, k_cap = t.k_cap;
    uint64_t* const legal = t.legal + (int64_t)row * words;
    for (int wd = lane; wd < words; wd += 64) legal[wd] = src.legal[(int64_t)e * words + wd];
    for (int k = lane; k < k_cap; k += 64) {
        t.best_order[(int64_t)row * k_cap + k] = 0;
        t.prior[(int64_t)row * k_cap + k] = root_prior ? root_prior[(int64_t)row * k_cap + k] : 0.0f;
    }
    int nl0 = __builtin_amdgcn_readfirstlane(src.nlegal[e]);
    if (nl0 > k_cap) nl0 = k_cap;          // (never: nlegal <= k_max <= k_cap)
    const XrTreeView v = {t.nodes + (int64_t)row * t.node_cap, t.rs + row, t.node_cap, k_cap, words, lane};
    if (lane == 0) {
        t.nlegal[row] = nl0;
        xr_tree_init_row(v, nl0);
    }
    __syncthreads();          // the copies and the root, before every lane reads them
    if (nl0 <= 0) return;          // a done env: no tree, no simulation
    xr_tree_expand_block(v, 0, legal, nullptr, nl0, t.has_prior ? t.prior + (int64_t)row * k_cap : nullptr);
}

// The first kernel of a session that continues ("XR-Tree v2, kept"): xr_tree_keep_begin_kernel's work on this pool.  t.nodes is the half
// the new session searches in, kp.old_nodes the half the last one searched in; the key's legal words are the last session's snapshot
// (kp.key_legal == t.legal), read before this kernel overwrites them with the env's current words.  A rebuilt row ends exactly as
// xr_tree_eval_open_kernel leaves it.
__global__ void __launch_bounds__(64) xr_tree_eval_reopen_kernel(XrBatchDev src, XrTreeEvalDev t, XrTreeKeepDev kp, const float* __restrict__ root_prior) {
#pragma clang fp contract(off)
    const int row = blockIdx.x, lane = threadIdx.x;
    const int e = t.env_lo + row;
    const int words = t.legal_words, k_cap = t.k_cap;
    XrTreeRow* const rs = t.rs + row;
    XrTreeNode* const nodes = t.nodes + (int64_t)row * t.node_cap;
    const XrTreeView v = {nodes, rs, t.node_cap, k_cap, words, lane};
    const XrTreeNode* const old = kp.old_nodes + (int64_t)row * t.node_cap;
    XrTreeKey* const key = kp.key + row;
    uint64_t* const snap = kp.key_legal + (int64_t)row * words;
    const uint64_t* const legal = src.legal + (int64_t)e * words;
    int nl0 = __builtin_amdgcn_readfirstlane(src.nlegal[e]);
    if (nl0 > k_cap) nl0 = k_cap;          // (never: nlegal <= k_max <= k_cap)
    const int64_t steps = src.env_steps[e];
    const int region = src.env_region[e], replay = src.env_replay[e];
    // 1. the key against the env, 2. the tree: the kept search's rules
    int child, used_old;
    const int a = kp.played ? __builtin_amdgcn_readfirstlane(kp.played[row]) : -1;
    const int mode = xr_tree_keep_mode(old, rs, key, snap, legal, words, a, nl0, steps, region, replay, t.node_cap, kp.n_add, lane, child, used_old);
    int kept_n, kept_nodes;
    xr_tree_keep_build(v, old, mode, child, used_old, nl0, src.reward + e, kept_n, kept_nodes);
    // 3. the session's snapshot (the next key's legal words), its row prior, an empty best line
    for (int wd = lane; wd < words; wd += 64) snap[wd] = legal[wd];
    for (int k = lane; k < k_cap; k += 64) {
        t.best_order[(int64_t)row * k_cap + k] = 0;
        t.prior[(int64_t)row * k_cap + k] = root_prior ? root_prior[(int64_t)row * k_cap + k] : 0.0f;
    }
    if (lane == 0) t.nlegal[row] = nl0;
    __syncthreads();          // the copies, before every lane reads them
    // 4. an unexpanded root (a rebuilt row's, or a kept child no simulation has left yet) gets its children under this call's prior
    if (nl0 > 0 && __builtin_amdgcn_readfirstlane(nodes[0].first) < 0)
        xr_tree_expand_block(v, 0, snap, nullptr, nl0, t.has_prior ? t.prior + (int64_t)row * k_cap : nullptr);
    // 5. the key of the state this tree belongs to
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

// dynamic LDS: XrTreePath
__global__ void __launch_bounds__(64) xr_tree_eval_select_kernel(XrTreeEvalDev t, int32_t* __restrict__ paths_out, int32_t* __restrict__ leaf_out) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char tree_eval_smem[];
    const int row = blockIdx.x, lane = threadIdx.x;
    const int words = t.legal_words, k_cap = t.k_cap, n_par = t.n_par;
    const XrTreePath path = xr_tree_path(tree_eval_smem, words, k_cap);
    const int nl0 = __builtin_amdgcn_readfirstlane(t.nlegal[row]);
    int32_t* const pfx = t.prefix + (int64_t)row * n_par * k_cap;
    int32_t* const pout = paths_out ? paths_out + (int64_t)row * n_par * k_cap : nullptr;
    int32_t* const leaf = t.leaf + (int64_t)row * n_par * 2;
    int32_t* const lout = leaf_out ? leaf_out + (int64_t)row * n_par * 2 : nullptr;
    if (nl0 <= 0) {              // a done row: empty paths (the peek launch answers them with the env's current state), no leaf
        xr_tree_empty_prefixes(pfx, pout, (int64_t)n_par * k_cap, lane);
        for (int i = lane; i < n_par * 2; i += 64) {
            const int f = (i & 1) ? XR_TREE_LEAF_NONE : -1;
            leaf[i] = f;
            if (lout) lout[i] = f;
        }
        return;
    }
    const XrTreeView v = {t.nodes + (int64_t)row * t.node_cap, t.rs + row, t.node_cap, k_cap, words, lane};
    const uint64_t* const legal = t.legal + (int64_t)row * words;
    const float* const w = t.has_prior ? t.prior + (int64_t)row * k_cap : nullptr;
    const double mn = v.rs->mn, mx = v.rs->mx;          // (backup alone changes them)
    for (int j = 0; j < n_par; j++) {
        int depth;
        const int node = xr_tree_descend(v, t.E, t.e_max, mn, mx, path, depth);
        int flags = 0;
        if (depth >= nl0) flags = XR_TREE_LEAF_TERMINAL;
        else if (__builtin_amdgcn_readfirstlane(v.nodes[node].first) < 0 && xr_tree_expand_block(v, node, legal, path.mask, nl0 - depth, w))
            flags = XR_TREE_LEAF_FRESH;
        xr_tree_finish_lane(v, path, depth, pfx, pout, j);
        if (lane == 0) {
            leaf[j * 2] = node; leaf[j * 2 + 1] = flags;
            if (lout) { lout[j * 2] = node; lout[j * 2 + 1] = flags; }
        }
    }
}

__global__ void __launch_bounds__(64) xr_tree_eval_backup_kernel(XrTreeEvalDev t, const double* __restrict__ value, const float* __restrict__ leaf_prior,
                                                                 int sims, int32_t* __restrict__ visits_out, double* __restrict__ value_out,
                                                                 int32_t* __restrict__ info_out, int32_t* __restrict__ best_order_out,
                                                                 double* __restrict__ best_return_out, double* __restrict__ returns_out) {
#pragma clang fp contract(off)
    const int row = blockIdx.x, lane = threadIdx.x;
    const int k_cap = t.k_cap, n_par = t.n_par;
    xr_tree_clear_outputs(visits_out, value_out, best_order_out, info_out, best_return_out, row, k_cap, lane);
    if (__builtin_amdgcn_readfirstlane(t.nlegal[row]) <= 0) {          // a done row: v1's empty result
        if (returns_out)
            for (int j = lane; j < n_par; j += 64) returns_out[(int64_t)row * n_par + j] = 0.0;
        return;
    }
    const XrTreeView v = {t.nodes + (int64_t)row * t.node_cap, t.rs + row, t.node_cap, k_cap, t.legal_words, lane};
    XrTreeNode* const nodes = v.nodes;
    XrTreeRow* const rs = v.rs;
    int32_t* const best_order = t.best_order + (int64_t)row * k_cap;
    const int used = __builtin_amdgcn_readfirstlane(rs->used);          // (backup makes no node)
    double mn = rs->mn, mx = rs->mx, best = rs->best;
    for (int j = 0; j < n_par; j++) {
        const int leaf_node = __builtin_amdgcn_readfirstlane(t.leaf[((int64_t)row * n_par + j) * 2]);
        const int flags = __builtin_amdgcn_readfirstlane(t.leaf[((int64_t)row * n_par + j) * 2 + 1]);
        const double ret = t.ret[(int64_t)row * n_par + j];
        double G = ret;
        if (!(flags & XR_TREE_LEAF_TERMINAL)) {
            double x = value[(int64_t)row * n_par + j];
            if (!(x >= -1.7976931348623157e308 && x <= 1.7976931348623157e308)) x = 0.0;          // not finite counts as 0 (a NaN fails both tests)
            G = ret + x;
        }
        const int32_t* const pfx = t.prefix + ((int64_t)row * n_par + j) * k_cap;
        xr_tree_backup_sim(v, used, pfx, G, mn, mx);
        if ((flags & XR_TREE_LEAF_TERMINAL) && G > best) {          // only a terminal line's G is an episode return
            best = G;
            for (int k = lane; k < k_cap; k += 64) best_order[k] = pfx[k];
        }
        if (returns_out && lane == 0) returns_out[(int64_t)row * n_par + j] = G;
        // the evaluator's prior over the children of the leaf this lane expanded: the Prior rule on that lane's row
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
    xr_tree_write_root(v, used, visits_out, value_out, info_out, best_return_out, row, sims, best);
    if (best_order_out)
        for (int k = lane; k < k_cap; k += 64) best_order_out[(int64_t)row * k_cap + k] = best_order[k];
}
