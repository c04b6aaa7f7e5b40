// xr_peek.h — peek (xr_batch_peek): the state every env would be in after a line of play, as a packed state row, without stepping.
// Included by xr_kernels.hip after xr_rollout.h; no router source changes, and xr_rollout_kernel is not touched: peek is a kernel of its
// own with the same loops.
//
//   xr_peek_kernel   persistent launch.  xr_rollout_kernel's task and ply loops with the policy XR_ROLLOUT_STOP built in (task t = (row
//                    t / n_lines, line t % n_lines); the shadow slot, the prefix rules, the accumulation and the record are the rollout's),
//                    and after the last ply the whole workgroup packs the shadow slot into the task's row in xr_pack_state_kernel's
//                    format: header (region of the SOURCE env + region_base, the shadow's nlegal), the shadow's legal words, one
//                    occupancy bit per node from the region's blockages and the shadow's owner row.
// The batch's own rows are only ever read.  No workgroup waits for another one.  No floating point except thread 0's `ret`, no atomics
// beyond the task claim; every store is a plain vector store.
#pragma once

// ctr / next_ctr: the claim counter of this call and the other bank, as in xr_rollout_kernel (the pool's rollout counters: calls on one
// pool are ordered by the caller)
template <bool LDS_DIST, int ZCH>
__global__ void __launch_bounds__(1024, 4) xr_peek_kernel(XrBatchDev src, XrBatchDev sh, int env_lo, int n_tasks, int n_lines,
                                                           const int32_t* __restrict__ prefix, int prefix_stride, int max_plies,
                                                           uint32_t* __restrict__ ctr, uint32_t* __restrict__ next_ctr,
                                                           uint8_t* __restrict__ rows, int64_t row_bytes, int region_base,
                                                           int32_t* __restrict__ out, double* __restrict__ return_out,
                                                           uint64_t* __restrict__ hash_out, int32_t* __restrict__ order_out, int k_cap) {     // (the route kernel's register budget)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_task, s_net;
    const int tid = threadIdx.x, lane = tid & 63;
    const int s = blockIdx.x;
    const int words = src.legal_words;
    const int ow = (src.n_max + 63) >> 6;
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
        const int row = task / n_lines;
        const int e = env_lo + row;
        int32_t* const ord = order_out ? order_out + (int64_t)task * k_cap : nullptr;
        xr_shadow_load(src, e, sh, s, sh_owner, words, tid, ord, k_cap);
        __syncthreads();
        // thread 0's view of the line, as in xr_rollout_kernel: pk = next entry of the prefix; -1: the prefix is over, and so is the line
        const int32_t* __restrict__ pfx = prefix ? prefix + (int64_t)task * prefix_stride : nullptr;
        int pk = pfx ? 0 : -1;
        int plies = 0, st_acc = 0, plen = 0;
        double ret = 0.0;
        for (;;) {
            if (tid == 0) {
                int net = 0;
                if (pk >= 0 && sh.nlegal[s] > 0 && (max_plies == 0 || plies < max_plies)) {      // (everything routed: the rest of a prefix is ignored)
                    const int a = pk < prefix_stride ? pfx[pk] : 0;
                    if (a > 0) { net = a; pk++; }
                    else pk = -1;                                                                   // list terminator
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
                    if (ord && plies < k_cap) ord[plies] = net;
                    plies++;
                    plen += sh.path_len[s];
                    ret += sh.reward[s];
                }
            }
            // Every iteration of both loops ENDS at a barrier (xr_lookahead_kernel has the reason)
            __syncthreads();
        }
        // The barrier every exit of the ply loop has passed (the one after the pick; before it, the one that ended the last route's
        // iteration, or the one after xr_shadow_load) stands between the router's last stores to the shadow slot and the reads below.
        uint8_t* const prow = rows + (int64_t)task * row_bytes;
        uint64_t* const lg = reinterpret_cast<uint64_t*>(prow + 16);
        uint64_t* const occ = lg + words;
        const int r = src.env_region[e];
        const int RN = src.regions[r].N;
        if (tid == 0) {
            int32_t* o = out + (int64_t)task * 8;
            o[0] = sh.cum[3 * s] - src.cum[3 * e]; o[1] = sh.cum[3 * s + 1] - src.cum[3 * e + 1]; o[2] = sh.cum[3 * s + 2] - src.cum[3 * e + 2];
            o[3] = st_acc; o[4] = plies; o[5] = sh.nlegal[s]; o[6] = plen; o[7] = 0;
            if (return_out) return_out[task] = ret;
            if (hash_out) hash_out[task] = sh.hash[s];
            int32_t* hdr = reinterpret_cast<int32_t*>(prow);
            hdr[0] = r + region_base; hdr[1] = sh.nlegal[s]; hdr[2] = words; hdr[3] = ow;
        }
        for (int w = tid; w < words; w += blockDim.x) lg[w] = sh.legal[(int64_t)s * words + w];
        // xr_pack_state_kernel's scheme: eight nodes per lane (two 16-byte loads), eight lanes per 64-bit word.  The bound is rounded up
        // to the workgroup's size: every lane of every wave reaches the shuffles.
        const int16_t* __restrict__ nn = src.rg_node_net + src.regions[r].node_off;
        const int nchunk = ow << 3;
        const int cmax = (RN + 7) >> 3;
        const int bdim = blockDim.x;
        for (int c = tid; c < (nchunk + bdim - 1) / bdim * bdim; c += bdim) {
            uint32_t bits = 0;
            if (c < cmax) {
                const int4 vn = *reinterpret_cast<const int4*>(nn + (c << 3));
                const int4 vo = *reinterpret_cast<const int4*>(sh_owner + (c << 3));
                const uint32_t n4[4] = {(uint32_t)vn.x, (uint32_t)vn.y, (uint32_t)vn.z, (uint32_t)vn.w};
                const uint32_t o4[4] = {(uint32_t)vo.x, (uint32_t)vo.y, (uint32_t)vo.z, (uint32_t)vo.w};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    bits |= (uint32_t)(((n4[j] & 0xFFFFu) == 0xFFFFu) || (o4[j] & 0xFFFFu)) << (2 * j);
                    bits |= (uint32_t)(((n4[j] >> 16) == 0xFFFFu) || (o4[j] >> 16)) << (2 * j + 1);
                }
                const int left = RN - (c << 3);
                if (left < 8) bits &= (1u << left) - 1u;
            }
            uint64_t v = (uint64_t)bits << (8 * (lane & 7));
            v |= __shfl_xor(v, 1, 64); v |= __shfl_xor(v, 2, 64); v |= __shfl_xor(v, 4, 64);
            if ((lane & 7) == 0 && (c >> 3) < ow) occ[c >> 3] = v;
        }
        // the task ends at a barrier: the next task's xr_shadow_load overwrites the rows read above
        __syncthreads();
    }
}
