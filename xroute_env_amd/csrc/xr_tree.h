// xr_tree.h — tree search (xr_batch_tree_search, "XR-Tree v1" of include/xroute_hip.h): pUCT over net orderings with the tree in device
// memory.  Included by xr_kernels.hip after xr_rollout.h and xr_tree_core.h; no router source changes.  One wavefront per row (an env of
// the caller), one tree per row in the row's pool of node_cap nodes; a search is n_waves x {select, xr_rollout_kernel, backup}, all in
// stream order.  The tree's rules — expansion, the descent, the backup of a simulation, the root's results — are xr_tree_core.h's; what
// is this form's own: the tree reads the env's live nlegal and legal words, a simulation's G is its rollout's return, any simulation's
// line may become the best one, and the outputs are written once, after the last wave.
//
//   xr_tree_reset_kernel    clears the row's outputs and its search state, makes the root and expands it
//   xr_tree_select_kernel   the n_par lanes of one wave descend one after the other, a fresh leaf is expanded; each path is written as
//                           the prefix the rollout launch then plays
//   xr_tree_backup_kernel   simulations in lane order, min / max / best; after the last wave the root's visit counts and values
// Contraction is off in every function.  Thread 0 alone writes the fields of existing nodes and the row state; a new children block is
// written by the 64 lanes and read after a workgroup barrier (xr_tree_core.h).  The batch's own rows are only ever read, no workgroup
// waits for another one.
#pragma once

__global__ void __launch_bounds__(64) xr_tree_reset_kernel(XrBatchDev src, XrTreeDev t) {
#pragma clang fp contract(off)
    const int row = blockIdx.x, lane = threadIdx.x;
    const int e = t.env_lo + row;
    xr_tree_clear_outputs(t.visits_out, t.value_out, t.best_order_out, t.info_out, t.best_return_out, row, t.k_cap, lane);
    const XrTreeView v = {t.nodes + (int64_t)row * t.node_cap, t.rs + row, t.node_cap, t.k_cap, src.legal_words, lane};
    const int nl0 = __builtin_amdgcn_readfirstlane(src.nlegal[e]);
    if (lane == 0) xr_tree_init_row(v, nl0);
    __syncthreads();          // the root and the row state, before every lane reads them
    if (nl0 <= 0) return;          // a done env: no tree, no simulation
    xr_tree_expand_block(v, 0, src.legal + (int64_t)e * src.legal_words, nullptr, nl0, t.prior ? t.prior + (int64_t)row * t.k_cap : nullptr);
}

// dynamic LDS: XrTreePath
__global__ void __launch_bounds__(64) xr_tree_select_kernel(XrBatchDev src, XrTreeDev t, int wave) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char tree_smem[];
    const int row = blockIdx.x, lane = threadIdx.x;
    const int e = t.env_lo + row;
    const int words = src.legal_words, k_cap = t.k_cap, n_par = t.n_par;
    const XrTreePath path = xr_tree_path(tree_smem, words, k_cap);
    const int nl0 = __builtin_amdgcn_readfirstlane(src.nlegal[e]);
    int32_t* const pfx = t.prefix + (int64_t)row * n_par * k_cap;
    int32_t* const pout = t.paths_out ? t.paths_out + ((int64_t)row * t.n_sims + (int64_t)wave * n_par) * k_cap : nullptr;
    if (nl0 <= 0) {              // a done env: empty paths (the rollout launch answers them with the empty rollout)
        xr_tree_empty_prefixes(pfx, pout, (int64_t)n_par * k_cap, lane);
        return;
    }
    const XrTreeView v = {t.nodes + (int64_t)row * t.node_cap, t.rs + row, t.node_cap, k_cap, words, lane};
    const uint64_t* const legal = src.legal + (int64_t)e * words;
    const float* const w = t.prior ? t.prior + (int64_t)row * k_cap : nullptr;
    const double mn = v.rs->mn, mx = v.rs->mx;          // (backup alone changes them)
    for (int j = 0; j < n_par; j++) {
        int depth;
        const int node = xr_tree_descend(v, t.E, t.e_max, mn, mx, path, depth);
        if (depth < nl0 && __builtin_amdgcn_readfirstlane(v.nodes[node].first) < 0) xr_tree_expand_block(v, node, legal, path.mask, nl0 - depth, w);
        xr_tree_finish_lane(v, path, depth, pfx, pout, j);
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
    const XrTreeView v = {t.nodes + (int64_t)row * t.node_cap, t.rs + row, t.node_cap, k_cap, src.legal_words, lane};
    XrTreeRow* const rs = v.rs;
    const int used = __builtin_amdgcn_readfirstlane(rs->used);          // (backup makes no node)
    double mn = rs->mn, mx = rs->mx, best = rs->best;
    for (int j = 0; j < n_par; j++) {
        const double G = t.ret[(int64_t)row * n_par + j];          // the rollout's return from the env's current state
        xr_tree_backup_sim(v, used, t.prefix + ((int64_t)row * n_par + j) * k_cap, G, mn, mx);
        if (G > best) {
            best = G;
            if (t.best_order_out)
                for (int k = lane; k < k_cap; k += 64) t.best_order_out[(int64_t)row * k_cap + k] = t.order[((int64_t)row * n_par + j) * k_cap + k];
        }
        if (t.returns_out && lane == 0) t.returns_out[(int64_t)row * t.n_sims + (int64_t)wave * n_par + j] = G;
    }
    if (lane == 0) { rs->mn = mn; rs->mx = mx; rs->best = best; }
    if (last) xr_tree_write_root(v, used, t.visits_out, t.value_out, t.info_out, t.best_return_out, row, (wave + 1) * n_par, best);
}
