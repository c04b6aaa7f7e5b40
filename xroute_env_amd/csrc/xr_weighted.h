// xr_weighted.h — weighted net sampling ("XR-Pick v1" of include/xroute_hip.h): a legal net drawn with probability proportional to a
// caller-supplied int32 weight per net, exact in integers.  Included by xr_kernels.hip after xr_rollout.h; no router source changes, and
// xr_rollout_kernel is not touched: the weighted rollout is a kernel of its own with the same loop.
//
//   xr_weighted_pick            the pick, run by ONE wavefront (all 64 lanes, converged): lane i of chunk c owns net 64c + i + 1, its legal
//                               bit is bit i of legal word c, its weight one coalesced load.  A 32-bit wave prefix sum per chunk, a 64-bit running total
//                               across chunks, a ballot for the first lane past t.  Two passes over the chunks (total, then locate);
//                               the scan of the last non-empty chunk is kept, so a row of up to 64 nets takes one.  r % S once per
//                               pick.  No floating point, no LDS.
//   xr_weighted_action_kernel   one wavefront per env, four per workgroup: the pick of the env's own row (xr_batch_weighted_actions)
//   xr_rollout_weighted_kernel  xr_rollout_kernel's loop with the policy XR_ROLLOUT_WEIGHTED: wave 0 picks on the shadow row, lane 0
//                               publishes the net through s_net
#pragma once

// q(n) of XR-Pick v1: 0 for w <= 0, else min(w, XR_WEIGHT_MAX).  The sum over a chunk of 64 nets fits 31 bits
__device__ __forceinline__ uint32_t xr_weight_q(const int32_t w) { return w <= 0 ? 0u : (w > XR_WEIGHT_MAX ? (uint32_t)XR_WEIGHT_MAX : (uint32_t)w); }

// a 64-bit value that is the same in every lane, as a scalar: what depends on it branches on the scalar unit
__device__ __forceinline__ uint64_t xr_uniform64(const uint64_t v) {
    return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v) |
           (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32;
}

// The pick of one env by one wavefront; every lane returns it.  `row` is where the state is read (the env's own slot, or a shadow slot
// that holds a copy of it), `env_id` the global env index the hash is keyed with, as in xr_random_pick: the same bits r.  w: the env's
// weight row, net n at n - 1, k_cap entries (entries of nets that are not legal are never read)
__device__ __forceinline__ int xr_weighted_pick(const XrBatchDev& b, const int row, const int env_id, const uint64_t seed, const int32_t* __restrict__ w,
                                                const int k_cap, const int lane) {
    const int words = b.legal_words;
    const uint64_t* __restrict__ lw = b.legal + (int64_t)row * words;
    // pass 1: the 32-bit wave prefix sum of q per chunk; its last lane is the chunk's total.  S = the sum of the totals, L = the number of
    // legal nets.  The scan of the LAST non-empty chunk stays in registers: rows of up to 64 nets never run pass 2
    uint64_t S = 0, base_keep = 0;
    uint32_t incl_keep = 0;
    int L = 0, c_keep = 0;
    for (int c = 0; c < words; c++) {
        const uint64_t m = xr_uniform64(lw[c]);
        if (m == 0) continue;
        L += __popcll(m);
        const int k = c * 64 + lane;
        uint32_t incl = (((m >> lane) & 1ULL) && k < k_cap) ? xr_weight_q(w[k]) : 0u;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t u = __shfl_up(incl, off, 64);
            if (lane >= off) incl += u;
        }
        base_keep = S; incl_keep = incl; c_keep = c;
        S += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
    if (L == 0) return 0;
    // S == 0: every legal net counts 1, which is the uniform pick r % L of xr_random_pick
    const bool unit = S == 0;
    const uint64_t r = splitmix64(seed ^ splitmix64((uint64_t)env_id * 0x100000001B3ULL + xr_uniform64((uint64_t)b.env_steps[row])));
    const uint64_t t = xr_uniform64(r % (unit ? (uint64_t)L : S));
    if (!unit && t >= base_keep) {                   // t falls into the chunk whose scan was kept
        const uint32_t tl = (uint32_t)(t - base_keep);
        return c_keep * 64 + __ffsll((long long)__ballot(incl_keep > tl));          // 1-based bit position == 1-based net id
    }
    // pass 2 (an earlier chunk, or unit weights): the lowest legal net whose running sum exceeds t
    uint64_t base = 0;
    for (int c = 0; c < words; c++) {
        const uint64_t m = xr_uniform64(lw[c]);
        if (m == 0) continue;
        const int k = c * 64 + lane;
        const bool legal = (m >> lane) & 1ULL;
        uint32_t incl = !legal ? 0u : unit ? 1u : k < k_cap ? xr_weight_q(w[k]) : 0u;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t u = __shfl_up(incl, off, 64);
            if (lane >= off) incl += u;
        }
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        if (t - base < (uint64_t)total) {            // (t >= base always)
            const uint32_t tl = (uint32_t)(t - base);
            return c * 64 + __ffsll((long long)__ballot(incl > tl));
        }
        base += total;
    }
    return 0;          // (not reached: t < the sum of the chunk totals)
}

// actions[i], weights[i][.]: row i of the caller = env env_base + i (the whole batch, or one env group: xr_batch_weighted_actions)
__global__ void __launch_bounds__(256) xr_weighted_action_kernel(XrBatchDev b, const int32_t* __restrict__ weights, int k_cap, int32_t* __restrict__ actions,
                                                                 uint64_t seed) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);             // one wave per env
    const int e = b.env_base + i;
    if (e >= XR_ENV_END(b)) return;
    const int net = xr_weighted_pick(b, e, e, seed, weights + (int64_t)i * k_cap, k_cap, lane);
    if (lane == 0) actions[i] = net;
}

// xr_rollout_kernel with the policy XR_ROLLOUT_WEIGHTED: the same tasks, shadow slot, prefix, routes, accumulation and record; after the
// prefix the net is the XR-Pick of the shadow row under seed_r from the ROW's weights (shared by the row's rollouts).  Thread 0 keeps the
// rollout's state as there; it tells wave 0 whether the policy picks, wave 0 picks, lane 0 publishes.
template <bool LDS_DIST, int ZCH>
__global__ void __launch_bounds__(1024, 4) xr_rollout_weighted_kernel(XrBatchDev src, XrBatchDev sh, int env_lo, int n_tasks, int n_rollouts, uint64_t seed,
                                                                       const int32_t* __restrict__ prefix, int prefix_stride, int max_plies,
                                                                       uint32_t* __restrict__ ctr, uint32_t* __restrict__ next_ctr,
                                                                       int32_t* __restrict__ out, double* __restrict__ return_out,
                                                                       uint64_t* __restrict__ hash_out, int32_t* __restrict__ order_out, int k_cap,
                                                                       const int32_t* __restrict__ weights, int weights_k_cap) {     // (the route kernel's register budget)
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
        xr_shadow_load(src, e, sh, s, sh_owner, words, tid, ord, k_cap);
        __syncthreads();
        // thread 0's view of the rollout, as in xr_rollout_kernel: pk = next entry of the prefix; -1: the policy picks; -2: the rollout is over
        const uint64_t seed_r = seed + (uint64_t)r * 0x9E3779B97F4A7C15ULL;
        const int32_t* __restrict__ pfx = prefix ? prefix + (int64_t)task * prefix_stride : nullptr;
        const int32_t* __restrict__ wrow = weights + (int64_t)row * weights_k_cap;
        int pk = pfx ? 0 : -1;
        int plies = 0, st_acc = 0, plen = 0;
        double ret = 0.0;
        for (;;) {
            if (tid < 64) {                       // wave 0, whole: the branch is a scalar one
                int net = 0, pick = 0;
                if (tid == 0) {
                    if (sh.nlegal[s] > 0 && (max_plies == 0 || plies < max_plies)) {      // (everything routed: the rest of a prefix is ignored)
                        if (pk >= 0) {
                            const int a = pk < prefix_stride ? pfx[pk] : 0;
                            if (a > 0) { net = a; pk++; }
                            else pk = -1;                                                   // list terminator
                        }
                        pick = pk == -1;
                    }
                }
                if (__builtin_amdgcn_readfirstlane(pick)) net = xr_weighted_pick(sh, s, e, seed_r, wrow, weights_k_cap, tid);
                if (tid == 0) s_net = net;
            }
            __syncthreads();
            const int net = __builtin_amdgcn_readfirstlane(s_net);    // (uniform, as the task above)
            if (net == 0) break;
            xr_route_dispatch<LDS_DIST, ZCH>(sh, s, net, smem);
            __syncthreads();              // (the router's epilogue runs on one thread of its choice: its stores are visible to wave 0 from here)
            if (tid == 0) {
                const int st = sh.status[s];
                st_acc |= st;
                if (!(st & XR_ENV_BAD_ACTION)) {          // a real route; a rejected entry of the prefix is flagged and costs no ply
                    if (ord && plies < k_cap) ord[plies] = net;
                    plies++;
                    plen += sh.path_len[s];
                    ret += sh.reward[s];
                } else if (pk < 0) {
                    pk = -2;
                }
            }
            // Every iteration of both loops ENDS at a barrier (xr_rollout_kernel states the rule): thread 0's block above and wave 0's pick
            // at the top of the next iteration must not become one divergent region across the back edge.
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
