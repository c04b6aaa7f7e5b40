// xr_lookahead.h — lookahead (xr_batch_lookahead): what every candidate net of every env would cost, without stepping.  Included by
// xr_kernels.hip after the routers; no router source changes.
//
//   xr_lookahead_plan_kernel   one wave per env row: candidates = legal & mask (bits within the region's nets).  Reserves a run of the
//                              task list for the env (one atomic per env), writes one task per candidate and the {0, 0, 0, -1} / -inf fill
//                              of every other entry of the output tables; zeroes the counters of the NEXT call (two alternating banks).
//   xr_lookahead_kernel        persistent launch (as many workgroups as the chip holds).  Every workgroup owns one SHADOW SLOT: private rows
//                              for everything a router writes per env, reached through a copy of XrBatchDev whose slot rows (and
//                              total_steps, phase_cycles) point at them (auto_reset = 0, net_meas = null, obs_out = null).  Per task, claimed
//                              with one atomic on a global counter: xr_shadow_load the env into the shadow slot, run the SAME router instantiation the step
//                              takes (xr_route_dispatch) on the shadow slot, copy the shadow delta / status / reward to the task's entry.
// The batch's own rows are only ever read.  No workgroup waits for another one, so launches of different env groups (each with a pool of
// shadow slots and counters of its own) may share the chip in any interleaving.
#pragma once

#define XR_LOOK_NEG_INF (-__builtin_huge_val())

// task = row * k_max + (net - 1), row = env - env_lo.  ctr: this call's bank {tasks listed, next task}; next_ctr: the other bank.
__global__ void __launch_bounds__(256) xr_lookahead_plan_kernel(XrBatchDev b, int env_lo, int rows, const uint64_t* __restrict__ cand_mask,
                                                                int32_t* __restrict__ out, double* __restrict__ reward_out, int k_cap,
                                                                int k_max, uint32_t* __restrict__ tasks, uint32_t* __restrict__ ctr,
                                                                uint32_t* __restrict__ next_ctr) {
    if (blockIdx.x == 0 && threadIdx.x == 0) { next_ctr[0] = 0; next_ctr[1] = 0; }
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);           // one wave per env row
    if (row >= rows) return;
    const int e = env_lo + row;
    const int words = b.legal_words;
    const uint64_t* __restrict__ lw = b.legal + (int64_t)e * words;
    const uint64_t* __restrict__ mw = cand_mask ? cand_mask + (int64_t)row * words : nullptr;
    const int n_nets = b.nlegal[e] > 0 ? min(b.regions[b.env_region[e]].n_nets, k_max) : 0;     // (a done env has no candidates)
    // candidate word w of this env (uniform over the wave)
    auto cand_word = [&](int w) -> uint64_t {
        const int lo = w * 64;
        if (lo >= n_nets) return 0ULL;
        uint64_t m = lw[w];
        if (mw) m &= mw[w];
        if (n_nets - lo < 64) m &= (1ULL << (n_nets - lo)) - 1ULL;
        return m;
    };
    int total = 0;
    for (int w = 0; w < words; w++) total += __popcll(cand_word(w));
    uint32_t base = 0;
    if (lane == 0 && total > 0) base = atomicAdd(&ctr[0], (uint32_t)total);
    base = __shfl(base, 0, 64);
    int before = 0;                                                // candidates in the words below the current one
    for (int k0 = 0; k0 < k_cap; k0 += 64) {
        const int w = k0 >> 6;
        const uint64_t m = w < words ? cand_word(w) : 0ULL;
        const int k = k0 + lane;
        if (k < k_cap) {
            if ((m >> lane) & 1ULL) {
                tasks[base + before + __popcll(m & ((1ULL << lane) - 1ULL))] = (uint32_t)row * (uint32_t)k_max + (uint32_t)k;
            } else {
                int32_t* o = out + ((int64_t)row * k_cap + k) * 4;
                o[0] = 0; o[1] = 0; o[2] = 0; o[3] = -1;
                if (reward_out) reward_out[(int64_t)row * k_cap + k] = XR_LOOK_NEG_INF;
            }
        }
        before += __popcll(m);
    }
}

// Env e of src into shadow slot s of sh, by the whole workgroup (the caller's barrier comes after it): what a router reads of a slot before
// it writes it.  The owner row as 16-byte vectors (n_max is a multiple of 8 elements, rows are 16-byte aligned), legal words, thread 0's scalars.
// ord (null: none): a rollout's order row, zeroed HERE, before thread 0's scalars — after them the rollout kernel measured 1 % slower
__device__ __forceinline__ void xr_shadow_load(const XrBatchDev& src, const int e, const XrBatchDev& sh, const int s, int16_t* const sh_owner,
                                               const int words, const int tid, int32_t* const ord = nullptr, const int k_cap = 0) {
    const int N = src.regions[src.env_region[e]].N;
    const int4* s4 = reinterpret_cast<const int4*>(src.owner + (int64_t)e * src.n_max);
    int4* d4 = reinterpret_cast<int4*>(sh_owner);
    const int nvec = (N + 7) >> 3;
    for (int i = tid; i < nvec; i += blockDim.x) d4[i] = s4[i];
    for (int w = tid; w < words; w += blockDim.x) sh.legal[(int64_t)s * words + w] = src.legal[(int64_t)e * words + w];
    if (ord)
        for (int k = tid; k < k_cap; k += blockDim.x) ord[k] = 0;
    if (tid == 0) {
        sh.env_region[s] = src.env_region[e]; sh.env_replay[s] = src.env_replay[e];
        sh.nlegal[s] = src.nlegal[e];
        sh.cum[3 * s] = src.cum[3 * e]; sh.cum[3 * s + 1] = src.cum[3 * e + 1]; sh.cum[3 * s + 2] = src.cum[3 * e + 2];
        sh.hash[s] = src.hash[e];
        sh.env_steps[s] = src.env_steps[e];
    }
}

// src: the batch (read only).  sh: its shadow view — per-env rows of `grid` shadow slots, slot s = workgroup s.
template <bool LDS_DIST, int ZCH>
__global__ void __launch_bounds__(1024, 4) xr_lookahead_kernel(XrBatchDev src, XrBatchDev sh, int env_lo, const uint32_t* __restrict__ tasks,
                                                                uint32_t* __restrict__ ctr, int32_t* __restrict__ out,
                                                                double* __restrict__ reward_out, int k_cap, int k_max) {     // (the route kernel's register budget)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_task;
    const int tid = threadIdx.x;
    const int s = blockIdx.x;
    const int words = src.legal_words;
    int16_t* const sh_owner = sh.owner + (int64_t)s * sh.n_max;
    for (;;) {
        if (tid == 0) {
            const uint32_t t = atomicAdd(&ctr[1], 1u);
            s_task = t < ctr[0] ? (int)tasks[t] : -1;
        }
        __syncthreads();
        const int task = __builtin_amdgcn_readfirstlane(s_task);      // (uniform: the loop's exit is a scalar branch)
        if (task < 0) break;
        const int row = task / k_max, net = task - row * k_max + 1;
        const int e = env_lo + row;
        xr_shadow_load(src, e, sh, s, sh_owner, words, tid);          // the env's state into the shadow slot
        __syncthreads();
        xr_route_dispatch<LDS_DIST, ZCH>(sh, s, net, smem);
        __syncthreads();              // (the router's epilogue runs on one thread of its choice: its stores are visible to thread 0 from here)
        if (tid == 0) {
            int32_t* o = out + ((int64_t)row * k_cap + (net - 1)) * 4;
            o[0] = sh.delta[3 * s]; o[1] = sh.delta[3 * s + 1]; o[2] = sh.delta[3 * s + 2]; o[3] = sh.status[s];
            if (reward_out) reward_out[(int64_t)row * k_cap + (net - 1)] = sh.reward[s];
        }
        // The iteration ENDS at a barrier.  Without it thread 0's block above and its claim at the top of the next iteration are one
        // divergent region across the loop's back edge: the compiler lets the other 63 lanes of wave 0 take the back edge first, so the
        // wave reaches the next barrier, and every wave reads s_task, before lane 0 has claimed anything — the old task again, routed with
        // thread 0 masked off, which never ends.
        __syncthreads();
    }
}
