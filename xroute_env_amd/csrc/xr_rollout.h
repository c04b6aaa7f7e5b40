// xr_rollout.h — rollouts (xr_batch_rollout): every env's episode played to its end, n_rollouts times, without stepping.  Included by
// xr_kernels.hip after the routers and xr_lookahead.h; no router source changes.
//
//   xr_rollout_kernel   persistent launch (as many workgroups as the chip holds), the three things the tree already had in one loop: the
//                       SHADOW SLOT of xr_lookahead.h (one per workgroup: private rows for everything a router writes per env), the
//                       back-to-back route loop of xr_order_kernel, and the counter-hash pick of xr_random_action_kernel (xr_random_pick).
//                       Task t = (row t / n_rollouts, rollout t % n_rollouts), claimed with one atomic on a global counter — no task list,
//                       and consecutive tasks share an env, whose owner row is then L2-hot.  Per task: copy the env's owner row and scalars
//                       into the shadow slot; then ply by ply thread 0 takes the next net from the task's prefix or from the policy and
//                       publishes it through LDS, the workgroup routes it on the shadow slot with the SAME router instantiation the step
//                       takes (xr_route_dispatch), thread 0 accumulates; after the last ply thread 0 writes the task's record.
// The batch's own rows are only ever read.  No workgroup waits for another one, so launches of different env groups (each with a pool of
// shadow slots and counters of its own) may share the chip in any interleaving.
#pragma once

// ctr: this call's claim counter (zero on entry); next_ctr: the other bank, zeroed here for the next call on this pool (nobody reads it
// during this one: calls on one pool are ordered by the caller)
template <bool LDS_DIST, int ZCH>
__global__ void __launch_bounds__(1024, 4) xr_rollout_kernel(XrBatchDev src, XrBatchDev sh, int env_lo, int n_tasks, int n_rollouts, int policy,
                                                              uint64_t seed, const int32_t* __restrict__ prefix, int prefix_stride, int max_plies,
                                                              uint32_t* __restrict__ ctr, uint32_t* __restrict__ next_ctr,
                                                              int32_t* __restrict__ out, double* __restrict__ return_out,
                                                              uint64_t* __restrict__ hash_out, int32_t* __restrict__ order_out, int k_cap) {     // (the route kernel's register budget)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_task, s_net;
    const int tid = threadIdx.x;
    const int s = blockIdx.x;
    const int words = src.legal_words;
    int16_t* const sh_owner = sh.owner + (int64_t)s * sh.n_max;
    if (s == 0 && tid == 0) *next_ctr = 0;
    for (;;) {
        if (tid == 0) {
            const uint32_t t = atomicAdd(ctr, 1u);
            s_task = t < (uint32_t)n_tasks ? (int)t : -1;
        }
        __syncthreads();
        const int task = __builtin_amdgcn_readfirstlane(s_task);      // (uniform: the loop's exit is a scalar branch)
        if (task < 0) break;
        const int row = task / n_rollouts, r = task - row * n_rollouts;
        const int e = env_lo + row;
        int32_t* const ord = order_out ? order_out + (int64_t)task * k_cap : nullptr;
        // the env's state into the shadow slot, as xr_lookahead_kernel copies it; the task's order row starts as "nothing routed"
        xr_shadow_load(src, e, sh, s, sh_owner, words, tid, ord, k_cap);
        __syncthreads();
        // thread 0's view of the rollout.  pk: next entry of the prefix; -1: the prefix is over, the policy picks; -2: the rollout is over
        // (a pick of the policy that the router rejected — it cannot happen while legal and nlegal agree, and must not spin if they do not)
        const uint64_t seed_r = seed + (uint64_t)r * 0x9E3779B97F4A7C15ULL;
        const int32_t* __restrict__ pfx = prefix ? prefix + (int64_t)task * prefix_stride : nullptr;
        int pk = pfx ? 0 : -1;
        int plies = 0, st_acc = 0, plen = 0;
        double ret = 0.0;
        for (;;) {
            if (tid == 0) {
                int net = 0;
                if (sh.nlegal[s] > 0 && (max_plies == 0 || plies < max_plies)) {      // (everything routed: the rest of a prefix is ignored, as xr_order_kernel does)
                    if (pk >= 0) {
                        const int a = pk < prefix_stride ? pfx[pk] : 0;
                        if (a > 0) { net = a; pk++; }
                        else pk = -1;                                                   // list terminator
                    }
                    if (pk == -1 && policy == XR_ROLLOUT_RANDOM) net = xr_random_pick(sh, s, e, seed_r);
                }
                s_net = net;
            }
            __syncthreads();
            const int net = __builtin_amdgcn_readfirstlane(s_net);    // (uniform, as the task above)
            if (net == 0) break;
            xr_route_dispatch<LDS_DIST, ZCH>(sh, s, net, smem);
            __syncthreads();              // (the router's epilogue runs on one thread of its choice: its stores are visible to thread 0 from here)
            if (tid == 0) {
                const int st = sh.status[s];
                st_acc |= st;
                if (!(st & XR_ENV_BAD_ACTION)) {          // a real route; a rejected entry of the prefix is flagged and costs no ply
                    if (ord && plies < k_cap) ord[plies] = net;          // (plies < the region's nets <= k_max <= k_cap: every real route retires a legal net)
                    plies++;
                    plen += sh.path_len[s];
                    ret += sh.reward[s];
                } else if (pk < 0) {
                    pk = -2;
                }
            }
            // Every iteration of both loops ENDS at a barrier (xr_lookahead_kernel has the reason): thread 0's block above and its pick at
            // the top of the next iteration must not become one divergent region across the back edge.
            __syncthreads();
        }
        if (tid == 0) {
            int32_t* o = out + (int64_t)task * 8;
            o[0] = sh.cum[3 * s] - src.cum[3 * e]; o[1] = sh.cum[3 * s + 1] - src.cum[3 * e + 1]; o[2] = sh.cum[3 * s + 2] - src.cum[3 * e + 2];
            o[3] = st_acc; o[4] = plies; o[5] = sh.nlegal[s]; o[6] = plen; o[7] = 0;
            if (return_out) return_out[task] = ret;
            if (hash_out) hash_out[task] = sh.hash[s];
        }
        __syncthreads();
    }
}
