// Device write-bandwidth probe: what a pure-write kernel can sustain on this GPU as a function of footprint and of
// the store pattern.  Build: hipcc --offload-arch=gfx950 -O3 -o write_bw write_bw.hip ; run: ./write_bw (every row) or ./write_bw slabs
// (the slab-ticket rows only) or ./write_bw heads (slab tickets from 1 or 8 ticket heads)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef float f4 __attribute__((ext_vector_type(4)));
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

// grid-stride over the whole buffer (what a plain fill does)
template <bool NT>
__global__ void k_grid(f4* __restrict__ p, size_t n4) {
    const f4 v = {1.f, 2.f, 3.f, 4.f};
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        if (NT) __builtin_nontemporal_store(v, p + i); else p[i] = v;
    }
}
// one workgroup per contiguous chunk (what the step kernel does: one env = one 2.5 MB run)
template <bool NT>
__global__ void k_chunk(f4* __restrict__ p, size_t chunk4) {
    const f4 v = {1.f, 2.f, 3.f, 4.f};
    f4* q = p + (size_t)blockIdx.x * chunk4;
    for (size_t i = threadIdx.x; i < chunk4; i += blockDim.x) {
        if (NT) __builtin_nontemporal_store(v, q + i); else q[i] = v;
    }
}

// the fused step kernel's order: the workgroup owning a chunk (= env) of `planes` planes of plane4 float4 each writes
// 4 KB of plane 0, 4 KB of plane 1, ... then the next 4 KB of every plane
template <bool NT>
__global__ void k_rot(f4* __restrict__ p, int planes, int plane4) {
    const f4 v = {1.f, 2.f, 3.f, 4.f};
    f4* q = p + (size_t)blockIdx.x * planes * plane4;
    for (int cb = 0; cb < plane4; cb += blockDim.x) {
        const int i = cb + threadIdx.x;
        if (i < plane4)
            for (int pl = 0; pl < planes; pl++) {
                if (NT) __builtin_nontemporal_store(v, q + (size_t)pl * plane4 + i); else q[(size_t)pl * plane4 + i] = v;
            }
    }
}
// globally ordered tickets: a workgroup repeatedly takes the next `blk4`-float4 block of the whole buffer
template <bool NT>
__global__ void k_ticket(f4* __restrict__ p, size_t n4, int blk4, unsigned* __restrict__ counter) {
    const f4 v = {1.f, 2.f, 3.f, 4.f};
    __shared__ unsigned s_t;
    const size_t nblk = (n4 + blk4 - 1) / blk4;
    for (;;) {
        if (threadIdx.x == 0) s_t = atomicAdd(counter, 1u);
        __syncthreads();
        const size_t t = s_t;
        __syncthreads();
        if (t >= nblk) break;
        f4* q = p + t * blk4;
        const size_t lim = (t + 1) * (size_t)blk4 <= n4 ? blk4 : n4 - t * blk4;
        for (size_t i = threadIdx.x; i < lim; i += blockDim.x) {
            if (NT) __builtin_nontemporal_store(v, q + i); else q[i] = v;
        }
    }
}

// slab tickets in the step kernel's geometry: rows `stride` floats apart, a unit = 7 planes of N floats at float (2 + 7 * rank) * N
// of its row, units in address order (units[u] = row << 14 | rank, as the plan kernel lists them).  A ticket is T tiles of a unit
// (tile = 256 float4 groups = 4 KB of each of the 7 planes, planes in rotation), ticket t -> unit t / S, slab t % S; thread 0 keeps
// D claims in flight (a claim is consumed D tickets after it was issued).  The first ticket of a workgroup is static.
template <int T, int D>
__global__ void __launch_bounds__(256) k_slab(float* __restrict__ base, const unsigned* __restrict__ units, int nunits, size_t stride, int N,
                                              unsigned* __restrict__ counter) {
    constexpr int S = (9 + T - 1) / T;
    const f4 v = {1.f, 2.f, 3.f, 4.f};
    __shared__ unsigned s_t;
    const int tid = threadIdx.x;
    const unsigned total = (unsigned)nunits * S;
    const int ngrp = N >> 2;
    unsigned ring[D];
    ring[0] = blockIdx.x;
    if (tid == 0)
        for (int d = 1; d < D; d++) ring[d] = gridDim.x + atomicAdd(counter, 1u);
    for (;;) {
        if (tid == 0) s_t = ring[0];
        __syncthreads();
        const unsigned t = __builtin_amdgcn_readfirstlane(s_t);
        __syncthreads();
        if (t >= total) break;
        if (tid == 0) {
#pragma unroll
            for (int d = 0; d + 1 < D; d++) ring[d] = ring[d + 1];
            ring[D - 1] = gridDim.x + atomicAdd(counter, 1u);
        }
        const unsigned u = t / S, p = t % S;
        const unsigned ent = units[u];
        float* __restrict__ out = base + (size_t)(ent >> 14) * stride + (size_t)(2 + 7 * (ent & 0x3FFFu)) * N;
#pragma unroll
        for (int j = 0; j < T; j++) {
            const int g = ((int)p * T + j) * 256 + tid;
            if (g < ngrp) {
                float* __restrict__ pp = out + ((size_t)g << 2);
#pragma unroll
                for (int pl = 0; pl < 7; pl++) __builtin_nontemporal_store(v, (f4*)(pp + (size_t)pl * N));
            }
        }
    }
}

// The same writer with H ticket heads (1 or 8, each in a 128-byte line of its own) and one claim kept ahead.  Head h = blockIdx.x & 7
// hands out the dynamic tickets h, h + 8, h + 16, ...; a workgroup whose head is exhausted reads the other seven at once and moves on to
// the next one that has tickets left (xr_claim_head_ticket of the step kernel).  LATE: the claim is issued after the ticket's stores
// instead of before them.
template <int T, int H, bool LATE>
__global__ void __launch_bounds__(256) k_slab_heads(float* __restrict__ base, const unsigned* __restrict__ units, int nunits, size_t stride, int N,
                                                    unsigned* __restrict__ heads) {
    constexpr int S = (9 + T - 1) / T;
    const f4 v = {1.f, 2.f, 3.f, 4.f};
    __shared__ unsigned s_t;
    const int tid = threadIdx.x;
    const unsigned total = (unsigned)nunits * S, first = gridDim.x;
    const int ngrp = N >> 2;
    int hd = H == 1 ? 0 : (int)(blockIdx.x & 7);
    auto claim = [&]() -> unsigned {
        if (H == 1) return first + atomicAdd(heads, 1u);
        for (;;) {
            const unsigned t = first + 8u * atomicAdd(&heads[hd * 32], 1u) + (unsigned)hd;
            if (t < total) return t;
            unsigned c[7];
#pragma unroll
            for (int k = 1; k < 8; k++) c[k - 1] = __hip_atomic_load(&heads[((hd + k) & 7) * 32], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int nh = -1;
#pragma unroll
            for (int k = 7; k >= 1; k--)
                if (first + 8u * c[k - 1] + (unsigned)((hd + k) & 7) < total) nh = (hd + k) & 7;
            if (nh < 0) return total;
            hd = nh;
        }
    };
    unsigned nx = blockIdx.x;
    for (;;) {
        if (tid == 0) s_t = nx;
        __syncthreads();
        const unsigned t = __builtin_amdgcn_readfirstlane(s_t);
        __syncthreads();
        if (t >= total) break;
        if (!LATE && tid == 0) nx = claim();
        const unsigned u = t / S, p = t % S;
        const unsigned ent = units[u];
        float* __restrict__ out = base + (size_t)(ent >> 14) * stride + (size_t)(2 + 7 * (ent & 0x3FFFu)) * N;
#pragma unroll
        for (int j = 0; j < T; j++) {
            const int g = ((int)p * T + j) * 256 + tid;
            if (g < ngrp) {
                float* __restrict__ pp = out + ((size_t)g << 2);
#pragma unroll
                for (int pl = 0; pl < 7; pl++) __builtin_nontemporal_store(v, (f4*)(pp + (size_t)pl * N));
            }
        }
        if (LATE && tid == 0) nx = claim();
    }
}

template <int T, int H, bool LATE>
static void run_slab_heads(float* base, const unsigned* units, int nunits, size_t stride, int N, unsigned* heads, hipEvent_t e0, hipEvent_t e1) {
    const int grids[] = {512, 1024};
    for (int G : grids) {
        float best = 1e30f, worst = 0.f;
        for (int rep = 0; rep < 4; rep++) {
            CK(hipMemsetAsync(heads, 0, 8 * 128, 0));
            CK(hipEventRecord(e0));
            hipLaunchKernelGGL((k_slab_heads<T, H, LATE>), dim3(G), dim3(256), 0, 0, base, units, nunits, stride, N, heads);
            CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            if (rep > 0) { if (ms < best) best = ms; if (ms > worst) worst = ms; }
        }
        const double wr = (double)nunits * 7 * N * 4;
        printf("%5.1f GB  slab T=%d (%6.1f KB) heads=%d claim %-6s %4dx256  %8.3f ms  %6.2f TB/s  spread %.3f ms (%.1f %%)\n", wr / 1e9, T, T * 28.0, H,
               LATE ? "after" : "before", G, best, wr / best / 1e9, worst - best, 100.0 * (worst - best) / best);
    }
}

template <int T, int D>
static void run_slab(float* base, const unsigned* units, int nunits, size_t stride, int N, unsigned* ctr, hipEvent_t e0, hipEvent_t e1) {
    const int grids[] = {512, 1024};
    for (int G : grids) {
        float best = 1e30f, worst = 0.f;
        for (int rep = 0; rep < 4; rep++) {
            CK(hipMemsetAsync(ctr, 0, 4, 0));
            CK(hipEventRecord(e0));
            hipLaunchKernelGGL((k_slab<T, D>), dim3(G), dim3(256), 0, 0, base, units, nunits, stride, N, ctr);
            CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            if (rep > 0) { if (ms < best) best = ms; if (ms > worst) worst = ms; }
        }
        const double wr = (double)nunits * 7 * N * 4;
        printf("%5.1f GB  slab T=%d (%6.1f KB) D=%d %4dx256  %8.3f ms  %6.2f TB/s  spread %.3f ms (%.1f %%)\n", wr / 1e9, T,
               (T < 9 ? T * 28.0 : 241920 / 1024.0), D, G, best, wr / best / 1e9, worst - best, 100.0 * (worst - best) / best);
    }
}

// the step's own span: 4096 rows of (2 + 7 * 36) * 8640 floats (8.78 MB, 36 GB in all), 2..19 units per row (10.4 GB written)
static void slab_rows(hipEvent_t e0, hipEvent_t e1, bool heads_rows) {
    const int rows = 4096, N = 8640;
    const size_t stride = (size_t)(2 + 7 * 36) * N;
    std::vector<unsigned> h;
    for (int r = 0; r < rows; r++) {
        const int k = 2 + (int)(((unsigned)r * 2654435761u >> 16) % 18u);
        for (int j = 0; j < k; j++) h.push_back(((unsigned)r << 14) | (unsigned)j);
    }
    const int nunits = (int)h.size();
    float* base; unsigned *units, *ctr;
    if (hipMalloc(&base, rows * stride * 4) != hipSuccess) { printf("alloc of the 36 GB span failed\n"); return; }
    CK(hipMalloc(&units, h.size() * 4)); CK(hipMalloc(&ctr, 8 * 128));
    CK(hipMemcpy(units, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    printf("# slab tickets: %d units of %d B over %d rows %zu B apart, best of 3 timed launches (spread = worst - best)\n", nunits, 7 * N * 4, rows,
           stride * 4);
    if (heads_rows) {       // ./write_bw heads: T x heads x claim placement, one claim ahead, and hipMemset of the same byte count
#define HEADS_ROWS(T) run_slab_heads<T, 1, false>(base, units, nunits, stride, N, ctr, e0, e1); run_slab_heads<T, 1, true>(base, units, nunits, stride, N, ctr, e0, e1); \
                      run_slab_heads<T, 8, false>(base, units, nunits, stride, N, ctr, e0, e1); run_slab_heads<T, 8, true>(base, units, nunits, stride, N, ctr, e0, e1)
        HEADS_ROWS(3); HEADS_ROWS(2); HEADS_ROWS(1);
#undef HEADS_ROWS
        const size_t wr = (size_t)nunits * 7 * N * 4;
        float best = 1e30f, worst = 0.f;
        for (int rep = 0; rep < 4; rep++) {
            CK(hipEventRecord(e0)); CK(hipMemsetAsync(base, 0, wr, 0)); CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            if (rep > 0) { if (ms < best) best = ms; if (ms > worst) worst = ms; }
        }
        printf("%5.1f GB  hipMemset (contiguous)  %8.3f ms  %6.2f TB/s  spread %.3f ms\n", wr / 1e9, best, wr / best / 1e9, worst - best);
        CK(hipFree(base)); CK(hipFree(units)); CK(hipFree(ctr));
        return;
    }
    run_slab<9, 1>(base, units, nunits, stride, N, ctr, e0, e1);
    run_slab<9, 2>(base, units, nunits, stride, N, ctr, e0, e1);
    run_slab<9, 4>(base, units, nunits, stride, N, ctr, e0, e1);
    run_slab<3, 1>(base, units, nunits, stride, N, ctr, e0, e1);
    run_slab<3, 2>(base, units, nunits, stride, N, ctr, e0, e1);
    run_slab<3, 4>(base, units, nunits, stride, N, ctr, e0, e1);
    run_slab<1, 1>(base, units, nunits, stride, N, ctr, e0, e1);
    run_slab<1, 2>(base, units, nunits, stride, N, ctr, e0, e1);
    run_slab<1, 4>(base, units, nunits, stride, N, ctr, e0, e1);
    CK(hipFree(base)); CK(hipFree(units)); CK(hipFree(ctr));
}

int main(int argc, char** argv) {
    const double gbs[] = {4.0, 10.9, 36.0};
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    if (argc > 1 && argv[1][0] == 's') { slab_rows(e0, e1, false); return 0; }      // ./write_bw slabs: the slab-ticket rows only
    if (argc > 1 && argv[1][0] == 'h') { slab_rows(e0, e1, true); return 0; }       // ./write_bw heads: 1 or 8 ticket heads, claim before / after the stores
    for (double gb : gbs) {
        size_t bytes = (size_t)(gb * 1e9) & ~(size_t)((1 << 22) - 1);
        f4* p; if (hipMalloc(&p, bytes) != hipSuccess) { printf("alloc %.1f GB failed\n", gb); continue; }
        const size_t n4 = bytes / 16;
        const size_t chunk4 = (2u << 20) / 16 + 8192;             // ~2.1 MB per workgroup
        const int nchunks = (int)(n4 / chunk4);
        const int nrot = (int)(n4 / (37 * 2160));
        unsigned* ctr; CK(hipMalloc(&ctr, 4));
        struct { const char* name; int kind; } tests[] = {{"grid plain 2048x256", 0}, {"grid NT    2048x256", 1}, {"grid NT   16384x256", 2},
                                                          {"chunk plain  wg=256", 3}, {"chunk NT     wg=256", 4}, {"memset", 5},
                                                          {"rot37 plain  wg=256", 6}, {"rot37 NT     wg=256", 7},
                                                          {"ticket 34.5K plain", 8}, {"ticket 34.5K NT", 9}, {"ticket 138K NT", 10},
                                                          {"chunk plain wg=1024", 11}, {"rot37 plain wg=1024", 12}};
        for (auto& t : tests) {
            float best = 1e30f;
            for (int rep = 0; rep < 4; rep++) {
                CK(hipEventRecord(e0));
                switch (t.kind) {
                    case 0: hipLaunchKernelGGL(k_grid<false>, dim3(2048), dim3(256), 0, 0, p, n4); break;
                    case 1: hipLaunchKernelGGL(k_grid<true>, dim3(2048), dim3(256), 0, 0, p, n4); break;
                    case 2: hipLaunchKernelGGL(k_grid<true>, dim3(16384), dim3(256), 0, 0, p, n4); break;
                    case 3: hipLaunchKernelGGL(k_chunk<false>, dim3(nchunks), dim3(256), 0, 0, p, chunk4); break;
                    case 4: hipLaunchKernelGGL(k_chunk<true>, dim3(nchunks), dim3(256), 0, 0, p, chunk4); break;
                    case 5: CK(hipMemsetAsync(p, 0, bytes, 0)); break;
                    case 6: hipLaunchKernelGGL(k_rot<false>, dim3(nrot), dim3(256), 0, 0, p, 37, 2160); break;
                    case 7: hipLaunchKernelGGL(k_rot<true>, dim3(nrot), dim3(256), 0, 0, p, 37, 2160); break;
                    case 8: CK(hipMemsetAsync(ctr, 0, 4, 0)); hipLaunchKernelGGL(k_ticket<false>, dim3(2048), dim3(256), 0, 0, p, n4, 2160, ctr); break;
                    case 9: CK(hipMemsetAsync(ctr, 0, 4, 0)); hipLaunchKernelGGL(k_ticket<true>, dim3(2048), dim3(256), 0, 0, p, n4, 2160, ctr); break;
                    case 10: CK(hipMemsetAsync(ctr, 0, 4, 0)); hipLaunchKernelGGL(k_ticket<true>, dim3(2048), dim3(256), 0, 0, p, n4, 8640, ctr); break;
                    case 11: hipLaunchKernelGGL(k_chunk<false>, dim3(nchunks), dim3(1024), 0, 0, p, chunk4); break;
                    case 12: hipLaunchKernelGGL(k_rot<false>, dim3(nrot), dim3(1024), 0, 0, p, 37, 2160); break;
                }
                CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
                float ms; CK(hipEventElapsedTime(&ms, e0, e1));
                if (rep > 0 && ms < best) best = ms;
            }
            const double wr = (t.kind == 3 || t.kind == 4 || t.kind == 11) ? (double)nchunks * chunk4 * 16
                            : (t.kind == 6 || t.kind == 7 || t.kind == 12) ? (double)nrot * 37 * 2160 * 16 : (double)bytes;
            printf("%5.1f GB  %-22s %8.3f ms  %6.2f TB/s\n", gb, t.name, best, wr / best / 1e9);
        }
        CK(hipFree(p));
    }
    slab_rows(e0, e1, false);
    return 0;
}
