// xr_batch.cpp — host side of libxroute_hip.so: the C ABI declared in include/xroute_hip.h.
// Owns the device state of a batch of env slots and enqueues the gfx950 kernels of xr_kernels.hip.
// There is NO CPU fallback in this library: without a HIP device every compute entry point fails
// with XR_ERR_HIP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/xroute_hip.h"
#include "xr_device.h"

namespace {

thread_local std::string g_err;

int32_t fail(int32_t code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define XR_HIP(call)                                                                        \
    do {                                                                                    \
        hipError_t _e = (call);                                                             \
        if (_e != hipSuccess)                                                               \
            return fail(XR_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

constexpr size_t kLdsLimit = 160 * 1024;       // LDS per CU on gfx950
constexpr size_t kLdsStatic = 1280;            // static __shared__ of the route kernel (AP staging etc.)

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    hipError_t alloc(size_t count) {
        release();
        n = count;
        if (count == 0) return hipSuccess;
        return hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T));
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    ~DevBuf() { release(); }
};

// The kernels index per-env rows of the caller's buffers (actions, observation) by the ABSOLUTE slot; for an env group the base is
// shifted back by `elems` elements so that slot lo lands on element 0 of the caller's buffer.  Only addresses of the group's own slots
// are ever formed from it on the device.  (Integer arithmetic: the shifted address need not point into any object.)
template <class T>
T* shift_back(T* p, int64_t elems) {
    return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(p) - (uintptr_t)(elems * (int64_t)sizeof(T)));
}

// Which caller buffer holds the current observation of a set of slots (what the in-place form may build on): keyed on pointer, row
// stride AND dtype (uint8: xr_batch_step_observe_u8 / xr_batch_observation_u8, else fp32)
struct ObsValid {
    const void* ptr = nullptr;
    int64_t stride = 0;
    bool u8 = false;
    void clear() { ptr = nullptr; }
    void set(const void* p, int64_t s, bool u) { ptr = p; stride = s; u8 = u; }
    bool holds(const void* p, int64_t s, bool u) const { return ptr == p && stride == s && u8 == u; }
};

// window form of the LDS router (xr_dial3.h, WIN); x = 0: off
struct Window { int x = 0, y = 0, nmax = 0, margin = 0, ystep = 1; uint32_t m24_yz = 0, m24_z = 0, m24_mw = 0, s24 = 0; };

}  // namespace

struct xr_batch {
    xr_config cfg{};
    bool loaded = false;
    int n_regions = 0;
    int n_max = 0;          // padded max nodes per region (multiple of 8)
    int n_max_nodes = 0;    // true max N
    int n_lds = 0;          // padded distance-field words (odd strides), max over regions
    int lines_max = 0;      // worklist items (line, chunk of 8 nodes) of the sweep router, max over regions
    int zch = 0;            // 9 / 12 when all regions have that many layers
    int kzch = 0;           // template selector of the step kernels: zch, or -1 = bucketed-frontier router (xr_dial.h)
    int k_max = 0;
    int legal_words = 1;
    int path_cap = 0;
    int x_max = 0, y_max = 0;
    bool all_n_mult4 = true;
    bool all_n_mult16 = true;   // every region's N % 16 == 0: the uint8 unit writer needs no LDS (xr_unit_u8_aligned), else it keeps the net's masks there
    bool lds_dist = true;
    bool stream_ok = false;   // ids + 2 bytes/node of the largest region fit the LDS of the observation stream form
    size_t route_lds = 0;
    int route_threads = 256;
    // regions
    DevBuf<XrRegionDev> regions;
    DevBuf<uint32_t> rg_rec;
    DevBuf<int16_t> rg_node_net, rg_owner0;
    DevBuf<int32_t> coords, net_csr, ap_node, ap_feat, net_info;
    DevBuf<uint8_t> ap_flags;
    DevBuf<int16_t> ap_pin;
    DevBuf<int32_t> guide_csr;            // XR-Maze v2, optional (xr_batch_load_guides): boxes of (region, net), indexed like net_csr
    DevBuf<int16_t> guide_box;
    DevBuf<uint8_t> guide_mask;           // XR-Maze v2 with guide_cost > 0: static "outside the guide" bitmasks of every (region, net) (build_guide_masks)
    size_t guide_mask_bytes = 0;
    std::vector<int32_t> h_net_off, h_n_nets, h_dims;   // per region: R.net_off, n_nets, (X, Y, Z) — what xr_batch_load_guides validates against
    size_t h_csr_size = 0;
    DevBuf<uint64_t> legal0;
    // envs
    DevBuf<int32_t> env_region, env_replay, nlegal, cum, delta, status, path, path_len, sweeps, touched, route_order;
    DevBuf<uint8_t> net_work, net_meas;
    int route_slots = 0;         // workgroups of the route kernel the chip holds at once (0: not asked yet)
    DevBuf<int16_t> owner;
    DevBuf<uint64_t> legal, hash;
    DevBuf<double> reward;
    DevBuf<XrStepRecord> records;
    DevBuf<uint8_t> done, cls_scratch;
    DevBuf<int64_t> env_steps;
    DevBuf<long long> phase_cycles;
    DevBuf<unsigned long long> total_steps;
    DevBuf<uint32_t> dist_scratch, dg_field, dg_masks, dg_touch, dg_path;
    bool dial_big = false;
    Window win;
    DevBuf<unsigned short> list_scratch;
    // split observation
    DevBuf<int32_t> plan_region, plan_unit_net;
    DevBuf<uint32_t> plan_units, queue;         // queue: two banks of 4 counters (route tasks, units, planned units, -), alternating per call
    int queue_bank = 0;
    uint32_t* queue_last = nullptr;             // the bank of the last planning call (XR_FETCH_UNITS)
    int n_cus = 0, queue_blocks = 0, queue_blocks_sweep = 0;
    bool sweep_full = false;     // auto router: the full-rewrite queue launch of a large batch takes the line-segment sweeps
    size_t sweep_lds = 0;
    hipStream_t aux_stream = nullptr;
    std::vector<hipStream_t> region_streams;        // stream-per-region mode
    std::vector<hipEvent_t> region_events;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_w0 = nullptr, ev_w1 = nullptr;
    int last_obs_mode = 0;
    int last_obs_inplace = 0;
    int last_obs_sweeps = 0;
    ObsValid obs_valid;                         // buffer that holds the current observation of ALL env slots (in-place form)
    // env groups (xr_batch_set_groups): group g = slots [group_bounds[g], group_bounds[g + 1]); one group = the whole batch until set
    int n_groups = 1;
    int32_t group_bounds[XR_MAX_GROUPS + 1] = {};
    DevBuf<uint32_t> group_queue;               // [XR_MAX_GROUPS][2][4]: two banks of queue counters per group, alternating per group step
    int group_bank[XR_MAX_GROUPS] = {};
    ObsValid group_valid[XR_MAX_GROUPS];        // per group: buffer (row 0 = the group's first slot) that holds its observation
    // lookahead (xr_batch_lookahead): private memory of the callers that have used it — [0] the whole batch, [1 + g] env group g.  One pool =
    // the slot rows of look_grid shadow slots plus the two per-launch rows a router also writes (carve_slots), the task list and two banks
    // of {tasks listed, next task}.  Rollouts (xr_batch_rollout) play in the same shadow slots — calls on one pool are ordered by the
    // caller — with claim counters of their own: roll_ctr, two alternating banks of one counter
    struct LookPool {
        DevBuf<uint8_t> mem;
        DevBuf<uint32_t> tasks, ctr, roll_ctr;
        int bank = 0, roll_bank = 0;
        XrSlotRows rows{};
        unsigned long long* total_steps = nullptr;
        long long* phase_cycles = nullptr;
        void release() { mem.release(); tasks.release(); ctr.release(); roll_ctr.release(); bank = 0; roll_bank = 0; }
    } look[1 + XR_MAX_GROUPS];
    // branch (xr_batch_branch): the staging pool of a caller — [0] the whole batch, [1 + g] env group g — allocated on its first branch: one
    // slot of rows per row of the caller (a map may stage every row: a permutation without fixed points)
    struct BranchPool {
        DevBuf<uint8_t> mem;
        int rows = 0;
        XrSlotRows stg{};
        void release() { mem.release(); rows = 0; }
    } branch[1 + XR_MAX_GROUPS];
    // tree search (xr_batch_tree_search): the private memory of a caller, indexed like look[] — the trees, the search state of every row
    // and one wave's paths, orders, rollout records and returns in one allocation that only ever grows; and the exploration tables it has
    // uploaded, one per (c_init, c_base), each with the host copy its asynchronous upload reads (never rewritten, so no call waits for it)
    struct TreeTable {
        double c_init = 0, c_base = 0;
        std::vector<double> host;
        DevBuf<double> dev;
    };
    struct TreePool {
        DevBuf<uint8_t> mem;
        std::vector<std::unique_ptr<TreeTable>> tables;
        void release() { mem.release(); tables.clear(); }
    } tree[1 + XR_MAX_GROUPS];
    // kept trees (xr_batch_tree_search_keep): a pool of its own per caller, indexed like tree[].  `trees` holds what outlives a call — two
    // halves of rows x node_cap nodes (a call re-roots from the half the last call searched in, `half`, into the other one), the row
    // states, the keys and their legal words — and depends on the shape below alone; `scratch` holds one wave's arrays and only ever
    // grows, so a call with more lanes keeps the trees.  A call whose shape differs from the last one's rebuilds every row
    struct KeepPool {
        DevBuf<uint8_t> trees, scratch;
        std::vector<std::unique_ptr<TreeTable>> tables;          // E[0 .. XR_TREE_MAX_SIMS] per (c_init, c_base)
        int rows = 0, lo = -1, node_cap = 0, k_cap = 0, legal_words = 0, half = 0;
        void release() { trees.release(); scratch.release(); tables.clear(); rows = 0; lo = -1; node_cap = 0; k_cap = 0; legal_words = 0; half = 0; }
    } keep[1 + XR_MAX_GROUPS];
    // evaluated tree search (xr_batch_tree_open / _leaves / _backup): a pool of its own per caller, indexed like tree[].  One session lives
    // here from its open call on: the trees, the snapshot of the legal words, one wave's paths, line returns and leaf records (`d` is the
    // view the kernels get), and on the host the session's shape, its simulations so far and whether a wave waits for its backup.  A
    // session started by xr_batch_tree_reopen is `keyed`: its carve of `mem` holds two halves of nodes (d.nodes is halves[half], the one
    // the session searches in; the next reopen re-roots from it into the other one) and a key per row, and its shape (rows, lo and d's
    // n_par, node_cap, k_cap, legal_words) is what the next reopen compares before it lets `played` reach the kernel
    struct EvalPool {
        DevBuf<uint8_t> mem;
        std::vector<std::unique_ptr<TreeTable>> tables;          // E[0 .. max_sims] per (c_init, c_base, max_sims)
        XrTreeEvalDev d{};
        XrTreeNode* halves[2] = {nullptr, nullptr};
        XrTreeKey* key = nullptr;
        int rows = 0, lo = -1, max_sims = 0, sims = 0, half = 0;
        bool open = false, pending = false, keyed = false;
        void release() {
            mem.release(); tables.clear(); d = XrTreeEvalDev{}; halves[0] = halves[1] = nullptr; key = nullptr;
            rows = 0; lo = -1; max_sims = 0; sims = 0; half = 0; open = false; pending = false; keyed = false;
        }
    } eval[1 + XR_MAX_GROUPS];
    int look_grid = 0;                         // workgroups of the persistent lookahead launch the chip holds at once (0: not asked yet)
    XrBatchDev dev{};
    ~xr_batch() {
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
        if (ev_w0) (void)hipEventDestroy(ev_w0);
        if (ev_w1) (void)hipEventDestroy(ev_w1);
        if (aux_stream) (void)hipStreamDestroy(aux_stream);
        for (hipEvent_t ev : region_events) (void)hipEventDestroy(ev);
        for (hipStream_t s : region_streams) (void)hipStreamDestroy(s);
    }
};

namespace {

// the longest observation row: planes 0..1 and seven planes per net of the largest region (floats; bytes of the uint8 form)
int64_t full_row(const xr_batch* b) { return (2 + 7 * (int64_t)b->k_max) * b->n_max_nodes; }

// how the fp32 observation is stored into a caller's rows: 1 = aligned float4 (every N % 4 == 0), 2 = shifted float4 (any N), 0 = scalar
// (unaligned caller buffer)
int obs_store_mode(const xr_batch* b, const void* ptr, int64_t stride) {
    const bool aligned = stride % 4 == 0 && (reinterpret_cast<uintptr_t>(ptr) & 15) == 0;
    return aligned ? (b->all_n_mult4 ? 1 : (b->stream_ok ? 2 : 0)) : 0;
}

// The router variant of a launch: the batch's default, or (sweep: only where xr_batch::sweep_full) the line-segment sweeps the auto router
// takes for the full rewrite of a large batch
XrRouteVariant route_variant(const xr_batch* b, bool sweep = false) {
    if (sweep) return {1, b->zch, b->sweep_lds, b->route_threads};
    return {b->lds_dist ? 1 : 0, b->kzch, b->route_lds, b->route_threads};
}

// d becomes the view of env group `group`: its slots [lo, lo + env_count) alone.  Returns lo — the caller shifts its per-env buffers back
// by it (shift_back)
int group_view(const xr_batch* b, int group, XrBatchDev& d) {
    const int lo = b->group_bounds[group];
    d.env_base = lo; d.env_count = b->group_bounds[group + 1] - lo;
    return lo;
}

// A whole-batch call that changes env state: no caller buffer holds the current observation any more (batch-wide or per group).
void drop_obs_valid(xr_batch* b) {
    b->obs_valid.clear();
    for (ObsValid& v : b->group_valid) v.clear();
}

// `out` (row 0 = slot env_lo; rows of `stride` floats, or bytes when u8) now holds the observation of slots [env_lo, env_hi): mark the
// batch if those are all of them, and every group the range covers, its slice of it
void mark_obs_valid(xr_batch* b, const void* out, int64_t stride, bool u8, int env_lo, int env_hi) {
    const int64_t row_bytes = stride * (u8 ? 1 : (int64_t)sizeof(float));
    if (env_lo == 0 && env_hi == b->cfg.n_envs) b->obs_valid.set(out, stride, u8);
    for (int g = 0; g < b->n_groups; g++)
        if (env_lo <= b->group_bounds[g] && b->group_bounds[g + 1] <= env_hi)
            b->group_valid[g].set(static_cast<const char*>(out) + (b->group_bounds[g] - env_lo) * row_bytes, stride, u8);
}

// ---- the state rows of an env slot, listed once (with XrSlotRows itself and fill_dev) ---------------------------------------------
// f(row of a, the same row of b, elements per slot) for every row.  A, B: XrSlotRows or XrBatchDev (rows of the same names and types:
// xr_device.h), the same object twice where one is enough.  Every pool of slots is carved by this, every view of one in the other made by it
template <class A, class B, class F>
constexpr void for_each_slot_row(A& a, B& b, size_t n_max, size_t path_cap, size_t legal_words, F&& f) {
    f(a.owner, b.owner, n_max); f(a.path, b.path, path_cap); f(a.legal, b.legal, legal_words);
    f(a.hash, b.hash, 1); f(a.reward, b.reward, 1); f(a.env_steps, b.env_steps, 1); f(a.records, b.records, 1);
    f(a.cum, b.cum, 3); f(a.delta, b.delta, 3);
    f(a.nlegal, b.nlegal, 1); f(a.status, b.status, 1); f(a.path_len, b.path_len, 1); f(a.sweeps, b.sweeps, 1); f(a.touched, b.touched, 1);
    f(a.env_region, b.env_region, 1); f(a.env_replay, b.env_replay, 1); f(a.done, b.done, 1);
}
// the DISTINCT members it visits: a row listed twice counts once, so a row left out cannot hide behind it
constexpr size_t slot_row_count() {
    XrSlotRows r{};
    const void* seen[64] = {};
    size_t n = 0;
    for_each_slot_row(r, r, 0, 0, 0, [&](auto*& p, auto*&, size_t) {
        for (size_t i = 0; i < n; i++)
            if (seen[i] == &p) return;
        if (n < 64) seen[n++] = &p;
    });
    return n;
}
static_assert(sizeof(XrSlotRows) == slot_row_count() * sizeof(void*), "every row of XrSlotRows is listed in for_each_slot_row, once");

// the rows of `from` into `to` (each an XrSlotRows or an XrBatchDev): the one conversion between the two, pointer types checked row by row
template <class A, class B>
void copy_slot_rows(A& to, const B& from) {
    for_each_slot_row(to, from, 0, 0, 0, [](auto& t, auto& f, size_t) { t = f; });
}

// One allocation cut into arrays, each starting on a 16-byte boundary
struct Carver {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off += (bytes + 15) & ~(size_t)15; return o; }
    // the next array, `count` elements: with the allocation's base its pointer into p; without one, sizing only
    template <class T>
    void place(uint8_t* base, T*& p, size_t count) { const size_t o = take(count * sizeof(T)); if (base) p = reinterpret_cast<T*>(base + o); }
};

// `slots` slots of every state row
void carve_slots(const xr_batch* b, Carver& c, uint8_t* base, XrSlotRows& r, size_t slots) {
    for_each_slot_row(r, r, b->n_max, b->path_cap, b->legal_words, [&](auto*& p, auto*&, size_t per_slot) { c.place(base, p, slots * per_slot); });
}


// ---- xr_batch_load_regions, step by step: stage_regions (descriptors -> host tables + Extents), place_route (Extents -> RoutePlacement),
// commit_load (both -> xr_batch), alloc_batch, upload_batch, fill_dev -------------------------------------------------------------------

using MagicCache = std::map<uint64_t, uint64_t>;   // (divisor, limit) -> multiplier << 8 | shift (0xFF: none)

// exact 24-bit magics (largest shift whose multiplier and products fit, then checked for every n below `lim`)
bool magic24(MagicCache& cache, uint32_t dv, uint32_t lim, uint32_t& M, uint32_t& S) {
    const uint64_t key = ((uint64_t)dv << 32) | lim;
    auto it = cache.find(key);
    if (it != cache.end()) { M = (uint32_t)(it->second >> 8); S = (uint32_t)(it->second & 0xFF); return S != 0xFF; }
    bool found = false;
    if (lim <= (1u << 24))
        for (int sh = 31; sh >= 0 && !found; sh--) {
            const uint64_t m = (((uint64_t)1 << sh) + dv - 1) / dv;
            if (m >= (1u << 24) || (uint64_t)(lim > 0 ? lim - 1 : 0) * m >= ((uint64_t)1 << 32)) continue;
            bool ok = true;
            for (uint32_t nn = 0; nn < lim && ok; nn++) ok = (uint32_t)(((uint64_t)nn * m) >> sh) == nn / dv;
            if (ok) { M = (uint32_t)m; S = (uint32_t)sh; found = true; }
        }
    cache[key] = found ? (((uint64_t)M << 8) | S) : 0xFF;
    return found;
}

// What the router placement needs to know of the regions: maxima over them, and what holds for all of them
struct Extents {
    int n_max_nodes = 0, k_max = 0, x_max = 0, y_max = 0;
    int n_lds = 0;                 // padded distance-field words (odd strides), max over regions, a multiple of 8
    int z_min = 1 << 30, z_max = 0;
    int64_t edge_max = 0;          // longest edge of any region graph, the via included (range checks of xr_dial3.h)
    int64_t ext_max = 0;           // widest span of a region's tracks in x or y, DBU
    int items_max = 0;             // worklist items (line, chunk of 8 nodes) of the sweep router, max over regions
    bool mult4 = true, mult16 = true;   // every N % 4 / % 16 == 0
    bool div24_all = true;         // every region has its exact 24-bit division constants
    size_t gmask_bytes = 0;        // XR-Maze v2: bytes of the static guide masks of every (region, net) (XrRegionDev::gmask_off)
    int n_max() const { return (n_max_nodes + 7) & ~7; }
    int zch() const { return (z_min == z_max && (z_max == 9 || z_max == 12)) ? z_max : 0; }
    int legal_words() const { return std::max(1, (k_max + 63) / 64); }
};

// The static tables of the regions as the device will hold them, staged on the host
struct RegionStaging {
    std::vector<XrRegionDev> reg;
    std::vector<uint32_t> rec;
    std::vector<int32_t> coords, csr, ap_node, ap_feat;
    std::vector<int16_t> ap_pin;
    std::vector<uint8_t> net_work;       // per (region, net): predicted route work class (launch order of route-only launches)
    std::vector<int32_t> info;           // per (region, net): static facts for xr_dial3.h (XrBatchDev::net_info)
    std::vector<uint8_t> ap_flags;       // per access point: bit 0 = its pin sits in a closed pocket; bits 1..2 = heuristic slot
    std::vector<uint64_t> legal0;
    MagicCache magics;
    Extents ext;
};

int32_t check_desc(const xr_region_desc& d, int r) {
    if (d.dim_x < 1 || d.dim_y < 1 || d.dim_z < 1 || d.dim_z > XR_MAX_LAYERS)
        return fail(XR_ERR_RANGE, "region %d: dims %dx%dx%d out of range (z <= %d)", r, d.dim_x, d.dim_y, d.dim_z,
                    XR_MAX_LAYERS);
    if ((int64_t)d.dim_x * d.dim_y * d.dim_z > (int64_t)1 << 30) return fail(XR_ERR_RANGE, "region %d: too many nodes", r);
    if (!d.xs_host || !d.ys_host || !d.layer_dir_host || !d.nodes_host)
        return fail(XR_ERR_INVALID, "region %d: null array", r);
    if (d.n_nets < 0 || d.n_nets > XR_MAX_NETS) return fail(XR_ERR_RANGE, "region %d: n_nets %d", r, d.n_nets);
    // track coordinates within +-2^30 DBU, both ends included: a difference of two of them reaches 2^31 and does NOT fit int32, so the
    // span of each axis is bounded as well (below, once the tables are known to ascend)
    for (int i = 0; i < d.dim_x; i++)
        if (d.xs_host[i] < -(1 << 30) || d.xs_host[i] > (1 << 30)) return fail(XR_ERR_RANGE, "region %d: xs[%d] = %d outside +-2^30", r, i, d.xs_host[i]);
    for (int i = 0; i < d.dim_y; i++)
        if (d.ys_host[i] < -(1 << 30) || d.ys_host[i] > (1 << 30)) return fail(XR_ERR_RANGE, "region %d: ys[%d] = %d outside +-2^30", r, i, d.ys_host[i]);
    for (int i = 1; i < d.dim_x; i++)
        if (d.xs_host[i] <= d.xs_host[i - 1]) return fail(XR_ERR_INVALID, "region %d: xs not strictly increasing", r);
    for (int i = 1; i < d.dim_y; i++)
        if (d.ys_host[i] <= d.ys_host[i - 1]) return fail(XR_ERR_INVALID, "region %d: ys not strictly increasing", r);
    // XR_MAX_TRACK_SPAN: the routers other than xr_dial3.h keep coordinates relative to the first track, x4, in 32-bit words and take
    // them as int in the search heuristic, which adds an x and a y span: 2 * 4 * span < 2^31.  Edge lengths x4 (< 2^30) plus a
    // distance word (< XR_DIST_CAP * 4 < 2^29) plus both penalties x4 (< 2^25) then stay inside the word too.  Nothing is lost to
    // the spec: an edge of XR_DIST_CAP (< 2^27) or more is never crossed, whatever its length
    const int64_t span_x = (int64_t)d.xs_host[d.dim_x - 1] - d.xs_host[0], span_y = (int64_t)d.ys_host[d.dim_y - 1] - d.ys_host[0];
    if (span_x >= XR_MAX_TRACK_SPAN || span_y >= XR_MAX_TRACK_SPAN)
        return fail(XR_ERR_RANGE, "region %d: tracks span %lld DBU in %s, the routers take spans below 2^28 (XR_MAX_TRACK_SPAN)", r,
                    (long long)(span_x >= XR_MAX_TRACK_SPAN ? span_x : span_y), span_x >= XR_MAX_TRACK_SPAN ? "x" : "y");
    return XR_OK;
}

// Shape, initial metrics, layer directions, and what the frontier routers divide by: smallest edge length, flat-index decode constants.
// One pass over the track pitches serves w_min and the longest edge / widest span of the batch
void decode_constants(const xr_config& cfg, const xr_region_desc& d, XrRegionDev& R, MagicCache& magics, Extents& ext) {
    const int64_t n64 = (int64_t)d.dim_x * d.dim_y * d.dim_z;
    R.X = d.dim_x; R.Y = d.dim_y; R.Z = d.dim_z; R.N = (int)n64;
    R.n_nets = d.n_nets;
    R.m0[0] = d.metrics0[0]; R.m0[1] = d.metrics0[1]; R.m0[2] = d.metrics0[2];
    R.ldir_mask = 0;
    for (int z = 0; z < d.dim_z; z++)
        if (d.layer_dir_host[z]) R.ldir_mask |= (1u << z);
    int64_t e_min = cfg.via_cost, e_max = cfg.via_cost;
    for (int i = 1; i < d.dim_x; i++) { const int64_t e = (int64_t)d.xs_host[i] - d.xs_host[i - 1]; e_min = std::min(e_min, e); e_max = std::max(e_max, e); }
    for (int i = 1; i < d.dim_y; i++) { const int64_t e = (int64_t)d.ys_host[i] - d.ys_host[i - 1]; e_min = std::min(e_min, e); e_max = std::max(e_max, e); }
    R.w_min = std::max(1u, (uint32_t)e_min);
    ext.edge_max = std::max(ext.edge_max, e_max);
    ext.ext_max = std::max<int64_t>(ext.ext_max, std::max<int64_t>((int64_t)d.xs_host[d.dim_x - 1] - d.xs_host[0], (int64_t)d.ys_host[d.dim_y - 1] - d.ys_host[0]));
    const uint32_t yz = (uint32_t)d.dim_y * (uint32_t)d.dim_z, zz = (uint32_t)d.dim_z;
    R.magic_yz = yz >= 2 ? (uint32_t)((1ULL << 32) / yz) : 0xFFFFFFFFu;
    R.magic_z = zz >= 2 ? (uint32_t)((1ULL << 32) / zz) : 0xFFFFFFFFu;
    const uint32_t mwv = (uint32_t)((n64 + 31) / 32);
    R.magic_mw = mwv >= 2 ? (uint32_t)((1ULL << 32) / mwv) : 0xFFFFFFFFu;
    uint32_t s_yz = 0, s_z = 0, s_mw = 0;
    const bool okd = n64 < 65536 && magic24(magics, yz, (uint32_t)n64, R.m24_yz, s_yz) && magic24(magics, zz, yz, R.m24_z, s_z) &&
                     magic24(magics, std::max(1u, mwv), (uint32_t)n64, R.m24_mw, s_mw);
    R.s24 = s_yz | (s_z << 8) | (s_mw << 16) | ((okd ? 1u : 0u) << 24);
    if (!okd) ext.div24_all = false;
}

// Per-net access-point lists (counting sort by 1-based net id; flat order inside a net) with ap_pin and ap_feat.  cnt: the region's
// slice of net_csr (access points of net n: [cnt[n], cnt[n + 1]) from R.ap_off)
int32_t stage_access_points(const xr_region_desc& d, int r, XrRegionDev& R, RegionStaging& s, std::vector<int32_t>& cnt) {
    R.net_off = (int32_t)s.csr.size();
    R.ap_off = (int32_t)s.ap_node.size();
    cnt.assign(d.n_nets + 2, 0);
    for (int f = 0; f < R.N; f++) {
        const uint32_t rec = d.nodes_host[f];
        if (XR_REC_TYPE(rec) == XR_TYPE_ACCESS) {
            const int net1 = (int)XR_REC_NET1(rec);
            if (net1 < 1 || net1 > d.n_nets)
                return fail(XR_ERR_RANGE, "region %d node %d: ACCESS node with net id %d outside 1..%d", r, f, net1,
                            d.n_nets);
            cnt[net1 + 1]++;
        }
    }
    for (int n = 1; n <= d.n_nets + 1; n++) cnt[n] += cnt[n - 1];
    R.nlegal0 = 0;
    for (int n = 1; n <= d.n_nets; n++) {
        const int c = cnt[n + 1] - cnt[n];
        if (c > XR_MAX_AP_PER_NET)
            return fail(XR_ERR_RANGE, "region %d net %d: %d access points (max %d)", r, n, c, XR_MAX_AP_PER_NET);
        R.nlegal0 += (c > 0);
    }
    s.csr.insert(s.csr.end(), cnt.begin(), cnt.end());
    const size_t base = s.ap_node.size();
    s.ap_node.resize(base + cnt[d.n_nets + 1]);
    s.ap_pin.resize(base + cnt[d.n_nets + 1]);
    std::vector<int32_t> cur(cnt.begin(), cnt.end());
    for (int f = 0; f < R.N; f++) {
        const uint32_t rec = d.nodes_host[f];
        if (XR_REC_TYPE(rec) == XR_TYPE_ACCESS) {
            const int net1 = (int)XR_REC_NET1(rec);
            s.ap_node[base + cur[net1]] = f;
            s.ap_pin[base + cur[net1]] = (int16_t)XR_REC_PIN1(rec);
            cur[net1]++;
        }
    }
    // per access point: does it have an in-bounds axis neighbour that is an access point of the same net, any pin
    // (the reference's aliased direction planes, baseline/build_3Dgrid.py:125-138); static, so decided once here
    s.ap_feat.resize(s.ap_node.size());
    const int Yd = d.dim_y, Zd = d.dim_z, YZd = Yd * Zd;
    auto net_of = [&](int f) -> int {
        const uint32_t rr = d.nodes_host[f];
        return XR_REC_TYPE(rr) == XR_TYPE_ACCESS ? (int)XR_REC_NET1(rr) : 0;
    };
    for (size_t i = base; i < s.ap_node.size(); i++) {
        const int f = s.ap_node[i], n = net_of(f);
        const int z = f % Zd, y = (f / Zd) % Yd, x = f / YZd;
        const bool adj = (x + 1 < d.dim_x && net_of(f + YZd) == n) || (y > 0 && net_of(f - Zd) == n) || (x > 0 && net_of(f - YZd) == n) ||
                         (y + 1 < Yd && net_of(f + Zd) == n) || (z + 1 < Zd && net_of(f + 1) == n) || (z > 0 && net_of(f - 1) == n);
        s.ap_feat[i] = f | (adj ? (int32_t)0x80000000 : 0);
    }
    return XR_OK;
}

// Static facts of every net for the round-3 router: lowest pin, number of distinct pins, and which pins are ISOLATED — all
// access points of the pin sit in a pocket closed by BLOCKAGE nodes that holds no access point of another pin of the net.
// Such a pin can never be reached (nor reach anything): XR-Maze v1 charges one violation for it, and a router that has to
// find that out by searching explores the whole component first.  The pocket's boundary is static, so the flood (budget 64
// nodes; a larger pocket just counts as open, the result is the same) runs here, once, not in every route.
void stage_net_facts(const xr_region_desc& d, const XrRegionDev& R, RegionStaging& s, const std::vector<int32_t>& cnt) {
    s.info.resize(s.csr.size(), 0);
    s.ap_flags.resize(s.ap_node.size(), 0);
    const int Xd = d.dim_x, Yd = d.dim_y, Zd = d.dim_z, YZd = Yd * Zd;
    const int32_t* ap_node = s.ap_node.data() + R.ap_off;
    const int16_t* ap_pin = s.ap_pin.data() + R.ap_off;
    uint8_t* ap_flags = s.ap_flags.data() + R.ap_off;
    auto blocked = [&](int f) { return XR_REC_TYPE(d.nodes_host[f]) == XR_TYPE_BLOCKAGE; };
    std::vector<int> seen_pins, pocket;
    for (int n = 1; n <= d.n_nets; n++) {
        const int lo = cnt[n], hi = cnt[n + 1];
        if (hi <= lo) continue;
        seen_pins.clear();
        for (int i = lo; i < hi; i++)
            if (std::find(seen_pins.begin(), seen_pins.end(), (int)ap_pin[i]) == seen_pins.end()) seen_pins.push_back(ap_pin[i]);
        const int first = *std::min_element(seen_pins.begin(), seen_pins.end());
        int n_iso = 0, src_iso = 0;
        for (int pn : seen_pins) {
            pocket.clear();
            for (int i = lo; i < hi; i++) if (ap_pin[i] == pn) pocket.push_back(ap_node[i]);
            bool open_pocket = false;
            for (size_t k = 0; k < pocket.size() && !open_pocket; k++) {
                const int f = pocket[k], z = f % Zd, y = (f / Zd) % Yd, x = f / YZd;
                const bool vert = d.layer_dir_host[z] != 0;
                const int nb[4] = {vert ? (y + 1 < Yd ? f + Zd : -1) : (x + 1 < Xd ? f + YZd : -1),
                                   vert ? (y > 0 ? f - Zd : -1) : (x > 0 ? f - YZd : -1),
                                   z + 1 < Zd ? f + 1 : -1, z > 0 ? f - 1 : -1};
                for (int q = 0; q < 4; q++) {
                    if (nb[q] < 0 || blocked(nb[q])) continue;
                    if (std::find(pocket.begin(), pocket.end(), nb[q]) != pocket.end()) continue;
                    if (pocket.size() >= 64) { open_pocket = true; break; }
                    pocket.push_back(nb[q]);
                }
            }
            if (open_pocket) continue;
            bool other = false;                    // an access point of another pin of the net inside the pocket: reachable
            for (int i = lo; i < hi && !other; i++)
                if (ap_pin[i] != pn && std::find(pocket.begin(), pocket.end(), ap_node[i]) != pocket.end()) other = true;
            if (other) continue;
            for (int i = lo; i < hi; i++) if (ap_pin[i] == pn) ap_flags[i] = 1;
            if (pn == first) src_iso = 1; else n_iso++;
        }
        s.info[R.net_off + n] = (first & 0x3FFF) | ((int)seen_pins.size() << 14) | (n_iso << 22) | (src_iso << 30);
        // heuristic slot of every access point (bits 1..2 of ap_flags): pins in ascending id order, the lowest one (the first
        // component: never a target) aside, are dealt round-robin over the three pin boxes of xr_dial3.h's heuristic
        std::sort(seen_pins.begin(), seen_pins.end());
        for (int i = lo; i < hi; i++) {
            const int rank = (int)(std::find(seen_pins.begin(), seen_pins.end(), (int)ap_pin[i]) - seen_pins.begin());
            ap_flags[i] |= (uint8_t)(((rank + 2) % 3) << 1);         // rank 1 -> slot 0, 2 -> 1, 3 -> 2, 4 -> 0 ...
        }
    }
}

// predicted work of routing net n: extent of its access points (DBU; a layer of span counted as half a via) times
// (6 + pins) — the shape tools/lpt_probe.py fitted; only the ORDER of these numbers matters
void stage_work_guess(const xr_config& cfg, const xr_region_desc& d, const XrRegionDev& R, const RegionStaging& s, const std::vector<int32_t>& cnt,
                      std::vector<float>& work) {
    work.resize(s.csr.size(), 0.0f);
    const int Yd = d.dim_y, Zd = d.dim_z, YZd = Yd * Zd;
    for (int n = 1; n <= d.n_nets; n++) {
        const int lo = cnt[n], hi = cnt[n + 1];
        if (hi <= lo) continue;
        int x0 = 1 << 30, x1 = -1, y0 = 1 << 30, y1 = -1, z0 = 1 << 30, z1 = -1;
        uint64_t pins[4] = {0, 0, 0, 0};
        int npins = 0;
        for (int i = lo; i < hi; i++) {
            const int f = s.ap_node[R.ap_off + i], z = f % Zd, y = (f / Zd) % Yd, x = f / YZd;
            x0 = std::min(x0, x); x1 = std::max(x1, x); y0 = std::min(y0, y); y1 = std::max(y1, y);
            z0 = std::min(z0, z); z1 = std::max(z1, z);
            const int pn = s.ap_pin[R.ap_off + i] & 255;
            if (!((pins[pn >> 6] >> (pn & 63)) & 1)) { pins[pn >> 6] |= 1ull << (pn & 63); npins++; }
        }
        const double ext = (double)(d.xs_host[x1] - d.xs_host[x0]) + (double)(d.ys_host[y1] - d.ys_host[y0]) +
                           0.5 * cfg.via_cost * (z1 - z0) + R.w_min;
        work[R.net_off + n] = (float)(ext * (6 + npins));
    }
}

// Worklist items of the sweep router are (line, chunk of 8 nodes) pairs: x-tracks * ceil(X/8) + y-tracks * ceil(Y/8) + columns * (1 when
// every region has 9 / 12 layers, else ceil(Z/8)); each kind is addressed with 16 bits
int32_t count_worklist_items(const std::vector<XrRegionDev>& reg, Extents& ext) {
    for (size_t r = 0; r < reg.size(); r++) {
        const XrRegionDev& R = reg[r];
        int nv = 0;
        for (int z = 0; z < R.Z; z++) nv += (R.ldir_mask >> z) & 1u;
        const int chH = (R.X + 7) / 8, chV = (R.Y + 7) / 8, chC = ext.zch() ? 1 : (R.Z + 7) / 8;
        const int64_t itH = (int64_t)(R.Z - nv) * R.Y * chH, itV = (int64_t)nv * R.X * chV, itC = (int64_t)R.X * R.Y * chC;
        if (itH > 65536 || itV > 65536 || itC > 65536)
            return fail(XR_ERR_RANGE, "region %d: more than 65536 worklist items of one kind (%lld / %lld / %lld)", (int)r,
                        (long long)itH, (long long)itV, (long long)itC);
        ext.items_max = std::max(ext.items_max, (int)(itH + itV + itC));
    }
    return XR_OK;
}

// Validates the descriptors and stages every static table; touches no xr_batch
int32_t stage_regions(const xr_config& cfg, const xr_region_desc* regs, int n_regions, RegionStaging& s) {
    Extents& ext = s.ext;
    ext.edge_max = cfg.via_cost;
    s.reg.resize(n_regions);
    std::vector<int32_t> cnt;
    std::vector<float> work;             // per (region, net): predicted route work
    for (int r = 0; r < n_regions; r++) {
        const xr_region_desc& d = regs[r];
        if (const int32_t rc = check_desc(d, r)) return rc;
        XrRegionDev& R = s.reg[r];
        decode_constants(cfg, d, R, s.magics, ext);
        R.xs_off = (int32_t)s.coords.size();
        s.coords.insert(s.coords.end(), d.xs_host, d.xs_host + d.dim_x);
        R.ys_off = (int32_t)s.coords.size();
        s.coords.insert(s.coords.end(), d.ys_host, d.ys_host + d.dim_y);
        R.gmask_off = (int64_t)ext.gmask_bytes;
        R.gmask_stride = (int32_t)((((size_t)R.N + 7) / 8 + 15) & ~(size_t)15);
        R.pad0 = 0;
        ext.gmask_bytes += (size_t)R.gmask_stride * (size_t)std::max(d.n_nets, 0);
        // node records, padded to a multiple of 8 elements so that int16 planes stay 16-byte aligned
        R.node_off = (int64_t)s.rec.size();
        s.rec.insert(s.rec.end(), d.nodes_host, d.nodes_host + R.N);
        while (s.rec.size() % 8) s.rec.push_back(XR_TYPE_NORMAL);
        if (const int32_t rc = stage_access_points(d, r, R, s, cnt)) return rc;
        stage_net_facts(d, R, s, cnt);
        stage_work_guess(cfg, d, R, s, cnt, work);
        ext.n_max_nodes = std::max(ext.n_max_nodes, R.N);
        ext.k_max = std::max(ext.k_max, d.n_nets);
        ext.x_max = std::max(ext.x_max, d.dim_x);
        ext.y_max = std::max(ext.y_max, d.dim_y);
        if (R.N % 4) ext.mult4 = false;
        if (R.N % 16) ext.mult16 = false;
        // padded field: l = x*SX + y*SY + z, SY = Z|1, SX = (Y*SY)|1 (xr_route_kernel)
        const int64_t sy = d.dim_z | 1, sx = ((int64_t)d.dim_y * sy) | 1;
        const int64_t words = (int64_t)d.dim_x * sx;
        if (words > ((int64_t)1 << 30)) return fail(XR_ERR_RANGE, "region %d: too many nodes", r);
        ext.n_lds = std::max(ext.n_lds, (int)((words + 7) & ~(int64_t)7));
        ext.z_min = std::min(ext.z_min, d.dim_z); ext.z_max = std::max(ext.z_max, d.dim_z);
    }
    const int legal_words = ext.legal_words();
    // the observation kernels stage the ascending legal-id list in LDS (4 bytes per possible net)
    if ((size_t)legal_words * 64 * 4 + (size_t)(legal_words + 1) * 4 > 60 * 1024)
        return fail(XR_ERR_RANGE, "k_max %d too large for the observation kernel's LDS id list (max ~15000 nets)", ext.k_max);
    s.legal0.assign((size_t)n_regions * legal_words, 0);
    for (int r = 0; r < n_regions; r++) {
        s.reg[r].legal0_off = (int64_t)r * legal_words;
        const int32_t* csr = s.csr.data() + s.reg[r].net_off;
        for (int n = 1; n <= s.reg[r].n_nets; n++)
            if (csr[n + 1] > csr[n]) s.legal0[(size_t)r * legal_words + ((n - 1) >> 6)] |= 1ULL << ((n - 1) & 63);
    }
    // work classes 1..255 relative to the batch's largest prediction
    s.net_work.assign(s.csr.size(), 0);
    float wmax = 1.0f;
    for (float w : work) wmax = std::max(wmax, w);
    for (size_t i = 0; i < work.size(); i++)
        if (work[i] > 0.0f) s.net_work[i] = (uint8_t)(1 + std::min(254, (int)(254.0f * work[i] / wmax)));
    return count_worklist_items(s.reg, ext);
}

// Where and how the route tasks of every later launch run: one of the 12 <LDS_DIST, ZCH> instantiations and its launch shape
struct RoutePlacement {
    int zch = 0;              // 9 / 12 when all regions have that many layers
    int kzch = 0;             // template selector of the step kernels: zch (sweep router), or < 0 = a frontier router (XR_ZCH_*)
    bool lds_dist = true;     // distance field in LDS, else in HBM scratch
    bool dial_big = false;    // the frontier router's HBM-scratch form (xr_dial.h)
    size_t route_lds = 0;
    int route_threads = 256;
    bool sweep_full = false;  // auto router: the full-rewrite queue launch of a large batch takes the line-segment sweeps
    size_t sweep_lds = 0;
    bool stream_ok = false;   // ids + 2 bytes/node of the largest region fit the LDS of the observation stream form
    Window win;
    size_t lw_max = 0;        // words per item bitmask of the sweep router
    int items_max = 0;
    int path_cap = 0;
};

// The LDS router inside a window of the region first (xr_dial3.h, WIN; xr_config.window: > 0 = that many tracks at most — the
// largest square window <= it that fits LDS; 0 (default) and < 0 = off: measured no faster on BASELINE config 5):
// every region must have the same layer count and hold the window, rows of the state arrays must start on 16-byte boundaries
// wherever a window row may start, the arithmetic limits are those of the form.  win_lds: the window's LDS when one is found
Window choose_window(const xr_config& cfg, RegionStaging& s, size_t big_lds, size_t& win_lds) {
    const Extents& ext = s.ext;
    Window win;
    const bool v2cfg = cfg.guide_cost > 0 || cfg.maze_end_iter > 1;
    const int64_t pen_w = (int64_t)cfg.drc_cost * cfg.drc_unit;
    if (cfg.window <= 0 || v2cfg || ext.z_min != ext.z_max || ext.edge_max + pen_w >= XR3_STEP_LIMIT) return win;
    const int Zw = ext.z_max;
    int ystep = 1;
    while ((ystep * Zw) % 8) ystep *= 2;                 // rows start at y0 * Z elements: a multiple of 8 of them (16 bytes of int16)
    bool rows_ok = true;
    int xmin = 1 << 30, ymin = 1 << 30;
    for (const XrRegionDev& R : s.reg) {
        rows_ok = rows_ok && ((int64_t)R.Y * Zw) % 8 == 0;
        xmin = std::min(xmin, R.X); ymin = std::min(ymin, R.Y);
    }
    for (int w = std::min(cfg.window, std::min(xmin, ymin)); w >= 8 && rows_ok; w--) {
        if ((w * Zw) % 8) continue;                          // a chunk of 8 nodes never straddles two window rows
        const int64_t nw = (int64_t)w * w * Zw;
        const size_t wl = XR3_LDS_BYTES((nw + 7) & ~7, w, w);
        if (nw >= 65536 || std::max(wl, big_lds) + 2 * kLdsStatic > kLdsLimit || (int64_t)w * ext.edge_max >= XR3_EXTENT_LIMIT) continue;
        uint32_t myz, syz, mz, sz, mmw, smw;
        const uint32_t mwv = (uint32_t)((nw + 31) / 32);
        if (!magic24(s.magics, (uint32_t)(w * Zw), (uint32_t)nw, myz, syz) || !magic24(s.magics, (uint32_t)Zw, (uint32_t)std::max(w, 1) * Zw * 2, mz, sz) ||
            !magic24(s.magics, mwv, (uint32_t)nw, mmw, smw)) continue;
        win.x = w; win.y = w; win.nmax = (int)((nw + 7) & ~7); win.ystep = ystep;
        // tracks kept free around the net's box (the row alignment is checked per net).  A net whose box nearly fills the window
        // floods past its faces, fails its certificate and has paid for the attempt on top of the fallback: margins of 4 / 8 /
        // 13 / 18 tracks of a 52-track window send 27 / 33 / 48 / 68 % of BASELINE config 5's routes to the fallback
        // (profiles/r04_l_config5_window_form.txt)
        win.margin = std::max(1, std::min(4, w / 8));
        if (const char* em = getenv("XR_WINDOW_MARGIN")) win.margin = std::max(1, atoi(em));      // (A/B runs)
        win.m24_yz = myz; win.m24_z = mz; win.m24_mw = mmw; win.s24 = syz | (sz << 8) | (smw << 16);
        win_lds = wl;
        break;
    }
    return win;
}

// The router choice, whole: which form routes, with the field where, in how much LDS, with how many threads.  Writes no xr_batch.
//   sweep router (kzch = zch >= 0): field in LDS when field + edge-length tables + 3 item bitmasks + worklists (u16 item ids; the claim
//     bitmask aliases them) fit, else in HBM scratch
//   frontier router, LDS (kzch -1; -3 = round 3's form, xr_dial3.h): field + node bitmasks + edge tables in LDS — the default
//   frontier router, HBM scratch (kzch -1, dial_big): regions too large for LDS, or force_scratch_field; may try an LDS window first
//   -2 / -4: the instantiations of -1 / -3 with the XR-Maze v2 knobs compiled in
int32_t place_route(const xr_config& cfg, RegionStaging& s, RoutePlacement& p) {
    const Extents& ext = s.ext;
    const int n_max = ext.n_max(), legal_words = ext.legal_words();
    p.zch = ext.zch();
    p.items_max = ext.items_max;
    p.path_cap = cfg.path_cap > 0 ? cfg.path_cap : std::min(ext.n_max_nodes, 4096);
    p.lw_max = ((size_t)ext.items_max + 31) / 32 + 1;
    const size_t el_bytes = (size_t)(ext.x_max + 2 + ext.y_max + 2) * 4;
    const size_t list_bytes = std::max(((size_t)ext.items_max * 2 + 3) & ~(size_t)3, ((size_t)ext.n_lds / 32 + 1) * 4);
    const size_t sweep_need = (size_t)ext.n_lds * 4 + el_bytes + 3 * p.lw_max * 4 + list_bytes + 16;
    const bool sweep_fits = sweep_need + kLdsStatic <= kLdsLimit && !cfg.force_scratch_field;
    const size_t dial_lds = (size_t)n_max * 4 + 4 * ((size_t)n_max / 32 + 1) * 4 + el_bytes + 16;
    // HBM-scratch form: groups of 1024 nodes must fit the LDS group table
    const size_t big_lds = (size_t)XR_BIG_MAXG * 6 + (size_t)XR_BIG_CA * 4 + (size_t)XR_BIG_CN * 4 + 2 * (size_t)XR_BIG_CE * 8 + el_bytes + 16;
    const bool frontier = cfg.router != XR_ROUTER_SWEEP, big_ok = ((size_t)n_max / 1024 + 2) <= 1024;
    // workgroup size unless the caller asks: 256 with the field in LDS (4 waves; 4 workgroups per CU resident at 24x40x9), 1024 with the
    // sweep router's field in HBM scratch (latency-bound on memory: more items in flight per env)
    int threads = 256;
    if (frontier && !cfg.force_scratch_field && dial_lds + kLdsStatic <= kLdsLimit) {
        p.kzch = -1; p.lds_dist = true; p.route_lds = dial_lds;
    } else if (frontier && big_ok) {
        p.kzch = -1; p.lds_dist = false; p.dial_big = true; p.route_lds = big_lds;
        // (round 2, config 5: 256 threads 4.2-4.7 ms, 512: 3.7-3.9 ms.  Round 3, same box, ms per launch at 256 / 1024 / 4096 envs: 512 threads
        //  1.9 / 2.7 / 4.0, 1024 threads 1.8 / 2.4 / 6.5 — a wider workgroup shortens each route's rounds (wide frontiers) but only one
        //  fits a CU: it pays while the batch is at most ~4 routes per CU, i.e. while the launch is bound by its longest routes)
        hipDeviceProp_t prop;
        threads = hipGetDeviceProperties(&prop, cfg.device) == hipSuccess && cfg.n_envs <= 4 * prop.multiProcessorCount ? 1024 : 512;
        size_t win_lds = 0;
        p.win = choose_window(cfg, s, big_lds, win_lds);
        p.route_lds = std::max(p.route_lds, win_lds);
    } else {
        p.kzch = p.zch; p.lds_dist = sweep_fits; p.route_lds = sweep_fits ? sweep_need : el_bytes + 3 * p.lw_max * 4;
        threads = sweep_fits ? 256 : 1024;
    }
    p.route_threads = cfg.block_threads ? cfg.block_threads : threads;
    // round 3's LDS form (xr_dial3.h) where it applies: the field fits with its queues, node ids fit 16 bits, and its 27-bit distance
    // arithmetic cannot wrap: every distance that exists is below XR_DIST_CAP = 0x07F00000 (spec; a candidate at or above the cap is
    // never written), so a reached word + one edge with every penalty stays inside 32 bits while that step is < 2^20 (the x32
    // fixed point of the word); the x32 coordinate tables and the heuristic need a region that spans < 2^25 DBU
    const size_t d3_lds = XR3_LDS_BYTES(n_max, ext.x_max, ext.y_max);
    const int64_t pen_max = ((int64_t)cfg.drc_cost * cfg.drc_unit) << (cfg.maze_end_iter - 1);
    const bool range_ok = ext.edge_max + pen_max + cfg.guide_cost < XR3_STEP_LIMIT && ext.ext_max < XR3_EXTENT_LIMIT &&
                          (int64_t)cfg.via_cost * 32 < XR3_EXTENT_LIMIT;
    if (p.kzch == -1 && p.lds_dist && cfg.router != XR_ROUTER_DIAL_R2 && range_ok && n_max < 65536 && ext.div24_all &&
        d3_lds + kLdsStatic <= kLdsLimit) {
        p.kzch = -3;
        p.route_lds = d3_lds;
    }
    if (cfg.guide_cost > 0 || cfg.maze_end_iter > 1) {
        if (p.kzch >= 0)
            return fail(XR_ERR_RANGE, "xr_batch_load_regions: XR-Maze v2 (guide_cost / maze_end_iter) needs the frontier router "
                                      "(router != XR_ROUTER_SWEEP, regions within its limits)");
        p.kzch = p.kzch == -3 ? -4 : -2;
    }
    if (p.kzch >= 0 && (cfg.router == XR_ROUTER_DIAL || cfg.router == XR_ROUTER_DIAL_R2))
        return fail(XR_ERR_RANGE, "xr_batch_load_regions: XR_ROUTER_DIAL: the largest region (%d nodes) exceeds the frontier router's limits", n_max);
    // the fused observation epilogue stages the ascending legal-id list in the same LDS; the flat-stream observation (any N): ids + a
    // 16-bit feature per node
    const size_t ids_bytes = (size_t)(legal_words * 64 + ((legal_words + 1 + 3) & ~3)) * 4;
    const size_t stream_bytes = ids_bytes + (size_t)n_max * 2;
    p.stream_ok = stream_bytes <= 60 * 1024;
    const size_t obs_lds = p.stream_ok && !ext.mult4 ? stream_bytes : ids_bytes;
    p.route_lds = std::max(p.route_lds, obs_lds);
    // router = 0 (auto) picks per entry point the scheme measured faster for it: the frontier router everywhere, except the
    // FULL-rewrite queue launch of a very large batch, where the line-segment sweeps are ahead (same box, DESIGN.md §5.1:
    // 1.727-1.730 ms against 1.773-1.775 ms per 4096-env step; at 2048 envs the frontier router wins, 0.921 against 0.945-0.954 ms)
    // (round 3, same box: synthetic 24x40x9 regions 1.681 ms with the sweeps against 1.700 ms with the frontier router; the regions
    //  extracted from ispd18_test1 — unaligned planes, 3.5 pins per net, K up to 77: their step is bound by routing, not by the write
    //  stream — 2.40 ms against 2.05 ms: the sweeps are only chosen for aligned planes)
    p.sweep_lds = std::max(sweep_need, obs_lds);
    p.sweep_full = cfg.router == 0 && (p.kzch == -1 || p.kzch == -3) && p.lds_dist && sweep_fits && cfg.block_threads == 0 &&
                   cfg.n_envs >= 4096 && ext.mult4 && p.sweep_lds + kLdsStatic <= kLdsLimit;
    if (p.route_lds + kLdsStatic > kLdsLimit)
        return fail(XR_ERR_RANGE, "route kernel needs %zu bytes of LDS (line bitmasks of the largest region)", p.route_lds);
    return XR_OK;
}

// Every range check has passed: what the regions are and where they route becomes the batch's
void commit_load(xr_batch* b, int n_regions, const RegionStaging& s, const RoutePlacement& p) {
    const Extents& ext = s.ext;
    b->n_regions = n_regions;
    b->n_max_nodes = ext.n_max_nodes;
    b->n_max = ext.n_max();
    b->n_lds = ext.n_lds;
    b->lines_max = p.items_max;
    b->k_max = ext.k_max;
    b->legal_words = ext.legal_words();
    b->x_max = ext.x_max;
    b->y_max = ext.y_max;
    b->all_n_mult4 = ext.mult4;
    b->all_n_mult16 = ext.mult16;
    b->zch = p.zch; b->kzch = p.kzch; b->lds_dist = p.lds_dist; b->dial_big = p.dial_big;
    b->route_lds = p.route_lds; b->route_threads = p.route_threads;
    b->sweep_full = p.sweep_full; b->sweep_lds = p.sweep_lds; b->stream_ok = p.stream_ok;
    b->win = p.win;
    b->path_cap = p.path_cap;
    b->h_net_off.resize(n_regions); b->h_n_nets.resize(n_regions); b->h_dims.resize(3 * (size_t)n_regions);
    for (int r = 0; r < n_regions; r++) {
        b->h_net_off[r] = s.reg[r].net_off; b->h_n_nets[r] = s.reg[r].n_nets;
        b->h_dims[3 * r] = s.reg[r].X; b->h_dims[3 * r + 1] = s.reg[r].Y; b->h_dims[3 * r + 2] = s.reg[r].Z;
    }
    b->h_csr_size = s.csr.size();
    b->guide_mask_bytes = ext.gmask_bytes;
}

int32_t alloc_batch(xr_batch* b, const RegionStaging& s) {
    const size_t B = (size_t)b->cfg.n_envs, n_rec = s.rec.size(), n_csr = s.csr.size(), n_ap = std::max<size_t>(1, s.ap_node.size());
#define XR_ALLOC(buf, count)                                                                        \
    do {                                                                                            \
        hipError_t _e = (buf).alloc(count);                                                         \
        if (_e != hipSuccess)                                                                       \
            return fail(XR_ERR_NOMEM, "hipMalloc of %zu bytes failed: %s", (size_t)(count) * sizeof(*(buf).p), \
                        hipGetErrorString(_e));                                                     \
    } while (0)
    XR_ALLOC(b->regions, s.reg.size());
    XR_ALLOC(b->rg_rec, n_rec);
    XR_ALLOC(b->rg_node_net, n_rec);
    XR_ALLOC(b->rg_owner0, n_rec);
    XR_ALLOC(b->coords, s.coords.size());
    XR_ALLOC(b->net_csr, n_csr);
    XR_ALLOC(b->ap_node, n_ap);
    XR_ALLOC(b->ap_pin, n_ap);
    XR_ALLOC(b->ap_feat, n_ap);
    XR_ALLOC(b->legal0, s.legal0.size());
    XR_ALLOC(b->env_region, B);
    XR_ALLOC(b->env_replay, B);
    XR_ALLOC(b->nlegal, B);
    XR_ALLOC(b->cum, B * 3);
    XR_ALLOC(b->delta, B * 3);
    XR_ALLOC(b->status, B);
    XR_ALLOC(b->path, B * b->path_cap);
    XR_ALLOC(b->path_len, B);
    XR_ALLOC(b->sweeps, B);
    XR_ALLOC(b->touched, B);
    XR_ALLOC(b->route_order, B);
    XR_ALLOC(b->net_work, n_csr);
    XR_ALLOC(b->net_meas, n_csr);
    XR_ALLOC(b->net_info, n_csr);
    XR_ALLOC(b->ap_flags, n_ap);
    XR_ALLOC(b->owner, B * b->n_max);
    XR_ALLOC(b->legal, B * b->legal_words);
    XR_ALLOC(b->hash, B);
    XR_ALLOC(b->reward, B);
    XR_ALLOC(b->records, B);
    XR_ALLOC(b->done, B);
    XR_ALLOC(b->env_steps, B);
    XR_ALLOC(b->total_steps, 1);
    XR_ALLOC(b->phase_cycles, B * 8);
    XR_ALLOC(b->plan_region, B);
    XR_ALLOC(b->queue, 8);
    XR_ALLOC(b->group_queue, (size_t)XR_MAX_GROUPS * 8);
    XR_ALLOC(b->plan_units, B * std::max(1, b->k_max));
    XR_ALLOC(b->plan_unit_net, B * std::max(1, b->k_max));
    if (b->dial_big) {
        const size_t mwg = (size_t)b->n_max / 32 + 1;
        XR_ALLOC(b->dg_field, B * b->n_max);
        XR_ALLOC(b->dg_masks, B * 2 * mwg);
        XR_ALLOC(b->dg_touch, B * b->n_max);
        XR_ALLOC(b->dg_path, B * b->n_max * 2);
    } else if (!b->lds_dist) {
        XR_ALLOC(b->dist_scratch, B * b->n_lds);
        XR_ALLOC(b->cls_scratch, B * b->n_lds);
        XR_ALLOC(b->list_scratch, B * b->lines_max);
    }
#undef XR_ALLOC
    return XR_OK;
}

// Static tables up, env state to its start, node records ingested.  Returns after the stream has drained: the staging may die
int32_t upload_batch(xr_batch* b, const RegionStaging& s, hipStream_t st) {
    const size_t B = (size_t)b->cfg.n_envs;
    XR_HIP(hipMemcpyAsync(b->regions.p, s.reg.data(), s.reg.size() * sizeof(XrRegionDev), hipMemcpyHostToDevice, st));
    XR_HIP(hipMemcpyAsync(b->rg_rec.p, s.rec.data(), s.rec.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    XR_HIP(hipMemcpyAsync(b->coords.p, s.coords.data(), s.coords.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    XR_HIP(hipMemcpyAsync(b->net_csr.p, s.csr.data(), s.csr.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    XR_HIP(hipMemcpyAsync(b->net_work.p, s.net_work.data(), s.net_work.size(), hipMemcpyHostToDevice, st));
    XR_HIP(hipMemsetAsync(b->net_meas.p, 0, s.csr.size(), st));                  // nothing measured yet: the launch orders use the geometric guess
    XR_HIP(hipMemcpyAsync(b->net_info.p, s.info.data(), s.info.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (!s.ap_flags.empty()) XR_HIP(hipMemcpyAsync(b->ap_flags.p, s.ap_flags.data(), s.ap_flags.size(), hipMemcpyHostToDevice, st));
    if (!s.ap_node.empty()) {
        XR_HIP(hipMemcpyAsync(b->ap_node.p, s.ap_node.data(), s.ap_node.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        XR_HIP(hipMemcpyAsync(b->ap_pin.p, s.ap_pin.data(), s.ap_pin.size() * sizeof(int16_t), hipMemcpyHostToDevice, st));
        XR_HIP(hipMemcpyAsync(b->ap_feat.p, s.ap_feat.data(), s.ap_feat.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    XR_HIP(hipMemcpyAsync(b->legal0.p, s.legal0.data(), s.legal0.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    std::vector<int32_t> henv(B);
    for (size_t e = 0; e < B; e++) henv[e] = (int32_t)(e % s.reg.size());
    XR_HIP(hipMemcpyAsync(b->env_region.p, henv.data(), B * sizeof(int32_t), hipMemcpyHostToDevice, st));
    XR_HIP(hipMemsetAsync(b->env_replay.p, 0, B * sizeof(int32_t), st));
    XR_HIP(hipMemsetAsync(b->env_steps.p, 0, B * sizeof(int64_t), st));
    XR_HIP(hipMemsetAsync(b->total_steps.p, 0, sizeof(unsigned long long), st));
    XR_HIP(hipMemsetAsync(b->phase_cycles.p, 0, B * 8 * sizeof(long long), st));
    XR_HIP(hipMemsetAsync(b->nlegal.p, 0, B * sizeof(int32_t), st));
    XR_HIP(hipMemsetAsync(b->touched.p, 0, B * sizeof(int32_t), st));
    XR_HIP(hipMemsetAsync(b->route_order.p, 0, B * sizeof(int32_t), st));
    XR_HIP(hipMemsetAsync(b->records.p, 0, B * sizeof(XrStepRecord), st));
    XR_HIP(hipMemsetAsync(b->owner.p, 0, B * b->n_max * sizeof(int16_t), st));
    XR_HIP(hipMemsetAsync(b->path.p, 0, B * b->path_cap * sizeof(int32_t), st));
    if (b->dial_big) {      // the persistent CLEAN state of the scratch: field CLEAN, no open bits, word minima = infinity
        const size_t mwg = (size_t)b->n_max / 32 + 1;
        XR_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(b->dg_field.p), (int)0xFFFFFFFEu, B * b->n_max, st));
        for (size_t e = 0; e < B; e++) {
            XR_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(b->dg_masks.p + e * 2 * mwg), 0, mwg, st));
            XR_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(b->dg_masks.p + e * 2 * mwg + mwg), (int)0xFFFFFFFFu, mwg, st));
        }
    }
    std::vector<uint64_t> hhash(B, 0xcbf29ce484222325ULL);
    XR_HIP(hipMemcpyAsync(b->hash.p, hhash.data(), B * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    XR_HIP(hipMemsetAsync(b->queue.p, 0, 8 * sizeof(uint32_t), st));       // both banks start clean; from then on every plan zeroes the other bank
    b->queue_bank = 0; b->queue_last = b->queue.p;
    XR_HIP(hipMemsetAsync(b->group_queue.p, 0, (size_t)XR_MAX_GROUPS * 8 * sizeof(uint32_t), st));     // (the partition itself survives a reload)
    for (int g = 0; g < XR_MAX_GROUPS; g++) b->group_bank[g] = 0;
    XR_HIP(xr_launch_ingest(b->rg_rec.p, b->rg_node_net.p, b->rg_owner0.p, (int64_t)s.rec.size(), st));
    XR_HIP(hipStreamSynchronize(st));   // host staging vectors die here
    return XR_OK;
}

// The kernels' view of the batch (zeroed by the caller): every buffer, size and knob
void fill_dev(xr_batch* b, const RoutePlacement& p) {
    XrBatchDev& d = b->dev;
    d.regions = b->regions.p; d.rg_rec = b->rg_rec.p; d.rg_node_net = b->rg_node_net.p; d.rg_owner0 = b->rg_owner0.p;
    d.coords = b->coords.p; d.net_csr = b->net_csr.p; d.ap_node = b->ap_node.p; d.ap_pin = b->ap_pin.p; d.ap_feat = b->ap_feat.p; d.net_work = b->net_work.p; d.net_info = b->net_info.p;
    d.ap_flags = b->ap_flags.p; d.legal0 = b->legal0.p; d.guide_csr = nullptr; d.guide_box = nullptr;
    {   // measured launch order (round 5): on unless XR_NO_MEASURED_ORDER=1 (A/B switch; results never depend on the order)
        const char* off = getenv("XR_NO_MEASURED_ORDER");
        d.net_meas = (off && off[0] == '1') ? nullptr : b->net_meas.p;
        const char* ht = getenv("XR_HEAVY_CLASS"); const char* hm = getenv("XR_HEAVY_MULT");       // (experiment switches)
        d.heavy_class = std::min(255, std::max(0, ht ? atoi(ht) : 0)); d.heavy_mult = std::min(16, std::max(1, hm ? atoi(hm) : 2));   // (a width of 0 would spin a route to its round cap)
        d.meas_shift = b->lds_dist ? 13 : 15;       // class unit: 8 k cycles (LDS form: a route is 0.1-1.5 M cycles), 32 k (HBM-scratch form: up to 6 M)
    }
    d.n_regions = b->n_regions; d.n_envs = b->cfg.n_envs; d.n_max = b->n_max; d.n_lds = b->n_lds; d.lw_max = (int)p.lw_max; d.lines_max = p.items_max;
    d.x_max = b->x_max; d.y_max = b->y_max; d.legal_words = b->legal_words; d.path_cap = b->path_cap;
    d.env_region = b->env_region.p; d.env_replay = b->env_replay.p; d.owner = b->owner.p; d.legal = b->legal.p;
    d.nlegal = b->nlegal.p; d.cum = b->cum.p; d.delta = b->delta.p; d.reward = b->reward.p; d.done = b->done.p;
    d.status = b->status.p; d.path = b->path.p; d.path_len = b->path_len.p; d.hash = b->hash.p;
    d.env_steps = b->env_steps.p; d.total_steps = b->total_steps.p; d.sweeps = b->sweeps.p; d.touched = b->touched.p; d.records = b->records.p;
    // (round 3's LDS form, same-box A/B profiles/r03_l_ab_bucket_width.txt: 12 against 8 — route-only 512 / 4096 envs 0.211 / 0.381 ->
    //  0.203 / 0.372 ms, 512-env step 0.315 -> 0.306 ms; 16 the same, 24 slower; round 2's form and the HBM-scratch form keep 8)
    d.dial_mult = b->cfg.dial_mult > 0 ? b->cfg.dial_mult : ((b->kzch == -3 || b->kzch == -4) ? 12 : 8);
    d.dial_mult_big = b->cfg.dial_mult > 0 ? b->cfg.dial_mult : 8;
    d.round_cap = b->cfg.debug_round_cap;
    d.win_x = b->win.x; d.win_y = b->win.y; d.win_nmax = b->win.nmax; d.win_margin = b->win.margin; d.win_ystep = b->win.ystep;
    d.win_m24_yz = b->win.m24_yz; d.win_m24_z = b->win.m24_z; d.win_m24_mw = b->win.m24_mw; d.win_s24 = b->win.s24;
    d.guide_cost = b->cfg.guide_cost; d.guide_margin = b->cfg.guide_margin; d.maze_end_iter = b->cfg.maze_end_iter;
    d.dg_field = b->dg_field.p; d.dg_masks = b->dg_masks.p; d.dg_touch = b->dg_touch.p; d.dg_path = b->dg_path.p;
    d.dist_scratch = b->dist_scratch.p; d.cls_scratch = b->cls_scratch.p; d.list_scratch = b->list_scratch.p; d.phase_cycles = b->phase_cycles.p;
    d.obs_split_pm = 1000;
    d.obs_lds_bytes = (int32_t)std::min<size_t>(b->route_lds, 1u << 30);      // (every launch of the default router carries route_lds)
    d.plan_region = b->plan_region.p; d.plan_units = b->plan_units.p; d.plan_unit_net = b->plan_unit_net.p; d.queue = b->queue.p; d.queue_quota_pm = 750;
    d.via_cost = b->cfg.via_cost; d.pen_cost = b->cfg.drc_cost * b->cfg.drc_unit;
    d.max_route_count = b->cfg.max_route_count; d.auto_reset = b->cfg.auto_reset;
    d.w_violation = b->cfg.w_violation; d.w_via = b->cfg.w_via; d.w_wirelength = b->cfg.w_wirelength;
}

}  // namespace

extern "C" {

int32_t xr_abi_version(void) { return XR_ABI_VERSION; }
const char* xr_last_error(void) { return g_err.c_str(); }

void xr_config_default(xr_config* c) {
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->struct_size = (int32_t)sizeof(xr_config);
    c->device = 0;
    c->n_envs = 1;
    c->via_cost = 800;
    c->drc_cost = 8;           // ispd/ispd18_test1/run-net-ordering-training.tcl:3  -drc_cost 8
    c->drc_unit = 400;
    c->max_route_count = 10;   // examples/launch_training.py:28
    c->auto_reset = 0;
    c->path_cap = 0;
    c->block_threads = 0;
    c->force_scratch_field = 0;
    c->obs_mode = 0;
    c->obs_writer_blocks = 0;
    c->obs_split_permille = 0;
    c->router = 0;
    c->dial_mult = 0;
    c->guide_cost = 0;
    c->guide_margin = 0;
    c->maze_end_iter = 1;      // ispd/ispd18_test1/run-net-ordering-training.tcl:3 runs 3; XR-Maze v1 = 1
    c->stream_per_region = 0;
    c->obs_helper_blocks = 0;
    c->launch_order = 0;
    c->debug_round_cap = 0;
    c->window = 0;
    c->w_violation = 500.0;    // baseline/DQN/train_DQN.py:99
    c->w_via = 4.0;
    c->w_wirelength = 0.5;
}

int32_t xr_device_count(int32_t* n) {
    if (!n) return fail(XR_ERR_INVALID, "xr_device_count: null argument");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *n = 0; return fail(XR_ERR_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *n = c;
    return XR_OK;
}

int32_t xr_batch_create(const xr_config* cfg, xr_batch** out) {
    if (!cfg || !out) return fail(XR_ERR_INVALID, "xr_batch_create: null argument");
    if (cfg->struct_size != (int32_t)sizeof(xr_config))
        return fail(XR_ERR_INVALID, "xr_batch_create: xr_config.struct_size %d != %zu (ABI mismatch)", cfg->struct_size,
                    sizeof(xr_config));
    if (cfg->n_envs < 1) return fail(XR_ERR_INVALID, "xr_batch_create: n_envs must be >= 1");
    if (cfg->via_cost < 1 || cfg->drc_cost < 0 || cfg->drc_unit < 0 || cfg->max_route_count < 1)
        return fail(XR_ERR_INVALID, "xr_batch_create: via_cost >= 1, drc_cost/drc_unit >= 0, max_route_count >= 1");
    if ((int64_t)cfg->drc_cost * cfg->drc_unit >= (1 << 22) || cfg->via_cost >= (1 << 22))
        return fail(XR_ERR_RANGE, "xr_batch_create: via_cost and drc_cost*drc_unit must be < 2^22");
    if (cfg->launch_order < 0 || cfg->launch_order > 2) return fail(XR_ERR_INVALID, "xr_batch_create: launch_order must be 0, 1 or 2");
    if (cfg->obs_mode < 0 || cfg->obs_mode > XR_OBS_QUEUE || cfg->obs_writer_blocks < 0 || cfg->obs_split_permille < 0 || cfg->obs_split_permille > 1000)
        return fail(XR_ERR_INVALID, "xr_batch_create: obs_mode must be 0, XR_OBS_FUSED, XR_OBS_SPLIT or XR_OBS_QUEUE; obs_writer_blocks >= 0; obs_split_permille in 0..1000");
    if (cfg->router < 0 || cfg->router > XR_ROUTER_DIAL_R2 || cfg->dial_mult < 0 || cfg->dial_mult > 64)
        return fail(XR_ERR_INVALID, "xr_batch_create: router must be 0, XR_ROUTER_SWEEP, XR_ROUTER_DIAL or XR_ROUTER_DIAL_R2; dial_mult in 0..64");
    if (cfg->guide_cost < 0 || cfg->guide_cost >= (1 << 22) || cfg->guide_margin < 0 || cfg->maze_end_iter < 1 || cfg->maze_end_iter > 8 ||
        ((int64_t)cfg->drc_cost * cfg->drc_unit << (cfg->maze_end_iter - 1)) >= (1 << 22))
        return fail(XR_ERR_RANGE, "xr_batch_create: guide_cost in [0, 2^22), guide_margin >= 0, maze_end_iter in 1..8 with drc_cost*drc_unit << (maze_end_iter-1) < 2^22");
    if (cfg->stream_per_region < 0 || cfg->stream_per_region > 1 || (cfg->stream_per_region && cfg->n_envs > 64))
        return fail(XR_ERR_RANGE, "xr_batch_create: stream_per_region is 0 or 1 and needs n_envs <= 64");
    if (cfg->debug_round_cap < 0 || cfg->obs_helper_blocks < 0)
        return fail(XR_ERR_INVALID, "xr_batch_create: debug_round_cap and obs_helper_blocks must be >= 0");
    if (cfg->block_threads != 0 && (cfg->block_threads < 64 || cfg->block_threads > 1024 || cfg->block_threads % 64))
        return fail(XR_ERR_INVALID, "xr_batch_create: block_threads must be a multiple of 64 in [64, 1024]");
    int ndev = 0;
    XR_HIP(hipGetDeviceCount(&ndev));
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(XR_ERR_HIP, "xr_batch_create: device %d not present (%d HIP devices)", cfg->device, ndev);
    XR_HIP(hipSetDevice(cfg->device));
    xr_batch* b = new (std::nothrow) xr_batch();
    if (!b) return fail(XR_ERR_NOMEM, "xr_batch_create: out of host memory");
    b->cfg = *cfg;
    b->group_bounds[0] = 0;
    b->group_bounds[1] = cfg->n_envs;
    *out = b;
    return XR_OK;
}

int32_t xr_batch_destroy(xr_batch* b) {
    if (!b) return XR_OK;
    (void)hipSetDevice(b->cfg.device);
    delete b;
    return XR_OK;
}

static int32_t build_guide_masks(xr_batch* b, hipStream_t st);

int32_t xr_batch_load_regions(xr_batch* b, const xr_region_desc* regs, int32_t n_regions, void* stream) {
    if (!b || !regs || n_regions < 1) return fail(XR_ERR_INVALID, "xr_batch_load_regions: bad argument");
    XR_HIP(hipSetDevice(b->cfg.device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    // a reload invalidates the batch until it has completed: a failure midway must not leave `loaded` set over
    // freed or partly reallocated device buffers
    b->loaded = false;
    drop_obs_valid(b);
    b->n_cus = 0;
    b->route_slots = 0;
    for (xr_batch::LookPool& lp : b->look) lp.release();         // shadow slots are sized for the regions they were allocated under
    for (xr_batch::BranchPool& bp : b->branch) bp.release();     // and so are the staging rows of xr_batch_branch
    for (xr_batch::TreePool& tp : b->tree) tp.release();
    for (xr_batch::KeepPool& kp : b->keep) kp.release();
    for (xr_batch::EvalPool& ep : b->eval) ep.release();
    b->look_grid = 0;
    b->guide_csr.release(); b->guide_box.release(); b->guide_mask.release(); b->guide_mask_bytes = 0;        // guides belong to the regions they were loaded for
    memset(&b->dev, 0, sizeof(b->dev));

    RegionStaging staging;
    RoutePlacement place;
    if (const int32_t rc = stage_regions(b->cfg, regs, n_regions, staging)) return rc;
    if (const int32_t rc = place_route(b->cfg, staging, place)) return rc;
    commit_load(b, n_regions, staging, place);
    const size_t lds_top = std::max(place.route_lds, place.sweep_full ? place.sweep_lds : 0);
    if (lds_top > 64 * 1024) XR_HIP(xr_route_set_max_lds(lds_top));
    if (const int32_t rc = alloc_batch(b, staging)) return rc;
    if (const int32_t rc = upload_batch(b, staging, st)) return rc;
    if (!b->aux_stream) {
        XR_HIP(hipStreamCreateWithFlags(&b->aux_stream, hipStreamNonBlocking));
        XR_HIP(hipEventCreateWithFlags(&b->ev_fork, hipEventDisableTiming));
        XR_HIP(hipEventCreateWithFlags(&b->ev_join, hipEventDisableTiming));
        XR_HIP(hipEventCreate(&b->ev_w0));
        XR_HIP(hipEventCreate(&b->ev_w1));
    }
    fill_dev(b, place);
    b->loaded = true;
    return build_guide_masks(b, st);          // (the default guides: bounding box of every net's access points)
}

// XR-Maze v2 with guide_cost > 0 and the round-3 LDS router: the guide of every (region, net) as a static bitmask (xr_guide_mask_kernel) — from the
// boxes loaded last (xr_batch_load_guides) or the default guides.  Without it (no guide cost, another router form, or more than 2 GiB of masks)
// dev.guide_mask stays null and the router decides membership per route as before.
static int32_t build_guide_masks(xr_batch* b, hipStream_t st) {
    b->dev.guide_mask = nullptr;
    const char* off = getenv("XR_NO_GUIDE_MASK");       // (A/B switch: membership per route, round 4's form; results are the same)
    if (b->cfg.guide_cost <= 0 || b->kzch != -4 || b->guide_mask_bytes == 0 || b->guide_mask_bytes > ((size_t)1 << 31) || (off && off[0] == '1')) {
        b->guide_mask.release();
        return XR_OK;
    }
    if (b->guide_mask.n != b->guide_mask_bytes && b->guide_mask.alloc(b->guide_mask_bytes) != hipSuccess) {
        b->guide_mask.release();
        return XR_OK;                    // (no memory for the masks: the per-route form still applies)
    }
    // (a mask build that cannot run degrades like one that has no memory: the router decides membership per route, same results)
    if (xr_launch_guide_masks(&b->dev, b->guide_mask.p, b->k_max, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        b->guide_mask.release();
        return XR_OK;
    }
    b->dev.guide_mask = b->guide_mask.p;
    return XR_OK;
}

// XR-Maze v2, optional: the nets' global-route guides as boxes.  Indexed like net_csr (boxes of net n of region r:
// [guide_csr[R.net_off + n], guide_csr[R.net_off + n + 1]) into guide_box, 6 int16 per box); a net without boxes keeps the default
// guide (bounding box of its access points).  Replaces every guide loaded before; a reload of the regions drops them.
int32_t xr_batch_load_guides(xr_batch* b, const int32_t* const* box_off_host, const int16_t* const* boxes_host, void* stream) {
    if (!b) return fail(XR_ERR_INVALID, "xr_batch_load_guides: null batch");
    if (!b->loaded) return fail(XR_ERR_STATE, "xr_batch_load_guides: load regions first");
    XR_HIP(hipSetDevice(b->cfg.device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    // (everything is validated and staged BEFORE the batch is touched: a refused table, or one there is no device memory for, leaves
    //  the guides loaded before — boxes and static masks alike — exactly as they were)
    if (!box_off_host) {      // back to the default guides
        b->dev.guide_csr = nullptr; b->dev.guide_box = nullptr;
        b->guide_csr.release(); b->guide_box.release();
        return build_guide_masks(b, st);
    }
    std::vector<int32_t> csr(b->h_csr_size, 0);
    std::vector<int16_t> box;
    for (int r = 0; r < b->n_regions; r++) {
        const int K = b->h_n_nets[r], X = b->h_dims[3 * r], Y = b->h_dims[3 * r + 1], Z = b->h_dims[3 * r + 2];
        int32_t* c = csr.data() + b->h_net_off[r];                 // c[n] .. c[n + 1], n = 1 .. K (slot 0 unused, like net_csr)
        const int32_t* off = box_off_host[r];
        const int16_t* bx = boxes_host ? boxes_host[r] : nullptr;
        for (int n = 1; n <= K; n++) {
            c[n] = (int32_t)(box.size() / 6);
            if (!off) continue;
            const int lo = off[n - 1], hi = off[n];
            if (lo < 0 || hi < lo || hi - lo > XR_GUIDE_MAX_BOXES || (hi > lo && !bx))
                return fail(XR_ERR_RANGE, "xr_batch_load_guides: region %d net %d: %d boxes (0..%d, offsets ascending)", r, n, hi - lo, XR_GUIDE_MAX_BOXES);
            for (int i = lo; i < hi; i++) {
                const int16_t* g = bx + 6 * (size_t)i;     // x0, y0, x1, y1, z0, z1, inclusive
                if (g[0] < 0 || g[2] < g[0] || g[2] >= X || g[1] < 0 || g[3] < g[1] || g[3] >= Y || g[4] < 0 || g[5] < g[4] || g[5] >= Z)
                    return fail(XR_ERR_RANGE, "xr_batch_load_guides: region %d net %d box %d (%d,%d)-(%d,%d) layers %d..%d outside the %dx%dx%d grid",
                                r, n, i - lo, g[0], g[1], g[2], g[3], g[4], g[5], X, Y, Z);
                box.insert(box.end(), g, g + 6);
            }
        }
        c[K + 1] = (int32_t)(box.size() / 6);
    }
    DevBuf<int32_t> new_csr;
    DevBuf<int16_t> new_box;
    if (new_csr.alloc(csr.size()) != hipSuccess || new_box.alloc(std::max<size_t>(6, box.size())) != hipSuccess)
        return fail(XR_ERR_NOMEM, "xr_batch_load_guides: hipMalloc failed (the guides loaded before stay in force)");
    XR_HIP(hipMemcpyAsync(new_csr.p, csr.data(), csr.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (!box.empty()) XR_HIP(hipMemcpyAsync(new_box.p, box.data(), box.size() * sizeof(int16_t), hipMemcpyHostToDevice, st));
    XR_HIP(hipStreamSynchronize(st));   // host staging vectors die here; work enqueued earlier that reads the old tables has finished too
    std::swap(b->guide_csr.p, new_csr.p); std::swap(b->guide_csr.n, new_csr.n);       // (the old tables are freed when new_* go out of scope)
    std::swap(b->guide_box.p, new_box.p); std::swap(b->guide_box.n, new_box.n);
    b->dev.guide_csr = b->guide_csr.p; b->dev.guide_box = b->guide_box.p;
    return build_guide_masks(b, st);
}

int32_t xr_batch_assign(xr_batch* b, const int32_t* env_region_host) {
    if (!b || !env_region_host) return fail(XR_ERR_INVALID, "xr_batch_assign: null argument");
    if (!b->loaded) return fail(XR_ERR_STATE, "xr_batch_assign: load regions first");
    for (int e = 0; e < b->cfg.n_envs; e++)
        if (env_region_host[e] < 0 || env_region_host[e] >= b->n_regions)
            return fail(XR_ERR_RANGE, "xr_batch_assign: env %d -> region %d outside 0..%d", e, env_region_host[e],
                        b->n_regions - 1);
    XR_HIP(hipSetDevice(b->cfg.device));
    XR_HIP(hipMemcpy(b->env_region.p, env_region_host, (size_t)b->cfg.n_envs * sizeof(int32_t), hipMemcpyHostToDevice));
    XR_HIP(hipMemset(b->env_replay.p, 0, (size_t)b->cfg.n_envs * sizeof(int32_t)));
    return XR_OK;
}

int32_t xr_batch_sizes(const xr_batch* b, int32_t* n_envs, int32_t* n_regions, int32_t* n_max, int32_t* k_max,
                       int32_t* legal_words, int32_t* path_cap, int64_t* obs_env_stride) {
    if (!b) return fail(XR_ERR_INVALID, "xr_batch_sizes: null batch");
    if (!b->loaded) return fail(XR_ERR_STATE, "xr_batch_sizes: load regions first");
    if (n_envs) *n_envs = b->cfg.n_envs;
    if (n_regions) *n_regions = b->n_regions;
    if (n_max) *n_max = b->n_max;
    if (k_max) *k_max = b->k_max;
    if (legal_words) *legal_words = b->legal_words;
    if (path_cap) *path_cap = b->path_cap;
    // (a multiple of 32 floats: every env's row starts on a 128-byte line, which is what lets the writers of unaligned planes
    //  store whole lines — any stride >= (2+7*k_max)*n_max is accepted, this is the one to prefer)
    if (obs_env_stride) *obs_env_stride = ((int64_t)(2 + 7 * (int64_t)b->k_max) * (int64_t)b->n_max + 31) & ~(int64_t)31;
    return XR_OK;
}

int32_t xr_batch_reset(xr_batch* b, const uint8_t* mask_dev, int32_t rotate, void* stream) {
    if (!b) return fail(XR_ERR_INVALID, "xr_batch_reset: null batch");
    if (!b->loaded) return fail(XR_ERR_STATE, "xr_batch_reset: load regions first");
    XR_HIP(hipSetDevice(b->cfg.device));
    drop_obs_valid(b);
    XR_HIP(xr_launch_reset(&b->dev, mask_dev, rotate ? 1 : 0, static_cast<hipStream_t>(stream)));
    return XR_OK;
}

namespace {
// One launch over the env slots of d (all of them, or one env group: d.env_base / env_count), or — stream_per_region — one
// single-workgroup launch per slot on a pool of internal streams (fork from / join to the caller's stream with events; the host
// never waits).  actions_dev is indexed by the absolute slot (shift_back for a group).
int32_t launch_route_form(xr_batch* b, const XrBatchDev& d, const int32_t* actions_dev, hipStream_t st) {
    const int lo = d.env_base, n = XR_ENV_END(d) - d.env_base;
    if (!b->cfg.stream_per_region) {
        // launch order: longest predicted route first when the launch runs in more than one round of workgroups
        bool lpt = b->cfg.launch_order == 2;
        if (b->cfg.launch_order == 0) {
            if (b->route_slots == 0) {
                hipDeviceProp_t prop;
                XR_HIP(hipGetDeviceProperties(&prop, b->cfg.device));
                int per_cu = 0;
                size_t stat = 0;
                XR_HIP(xr_route_occupancy(route_variant(b), &per_cu, &stat));
                b->route_slots = std::max(1, per_cu) * prop.multiProcessorCount;
            }
            lpt = n > b->route_slots;
        }
        if (!lpt) {
            XR_HIP(xr_launch_route(&d, actions_dev, route_variant(b), st));
            return XR_OK;
        }
        XrBatchDev dl = d;
        XR_HIP(xr_launch_route_order(&dl, actions_dev, b->route_order.p + lo, st));
        dl.route_order = b->route_order.p + lo;
        XR_HIP(xr_launch_route(&dl, actions_dev, route_variant(b), st));
        return XR_OK;
    }
    if (b->region_streams.empty()) {
        const int ns = std::min(b->cfg.n_envs, 16);
        for (int i = 0; i < ns; i++) {
            hipStream_t s; hipEvent_t ev;
            XR_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
            XR_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            b->region_streams.push_back(s); b->region_events.push_back(ev);
        }
    }
    const int ns = (int)b->region_streams.size();
    XR_HIP(hipEventRecord(b->ev_fork, st));
    for (int i = 0; i < ns; i++) XR_HIP(hipStreamWaitEvent(b->region_streams[i], b->ev_fork, 0));
    for (int e = lo; e < lo + n; e++) {
        XrBatchDev de = d;
        de.env_base = e; de.env_count = 1;
        XR_HIP(xr_launch_route(&de, actions_dev, route_variant(b), b->region_streams[e % ns]));
    }
    for (int i = 0; i < ns; i++) {
        XR_HIP(hipEventRecord(b->region_events[i], b->region_streams[i]));
        XR_HIP(hipStreamWaitEvent(st, b->region_events[i], 0));
    }
    return XR_OK;
}
}  // namespace

int32_t xr_batch_step(xr_batch* b, const int32_t* actions_dev, void* stream) {
    if (!b || !actions_dev) return fail(XR_ERR_INVALID, "xr_batch_step: null argument");
    if (!b->loaded) return fail(XR_ERR_STATE, "xr_batch_step: load regions first");
    XR_HIP(hipSetDevice(b->cfg.device));
    drop_obs_valid(b);
    return launch_route_form(b, b->dev, actions_dev, static_cast<hipStream_t>(stream));
}

namespace {
// group < 0: the whole batch (xr_batch_step_observe*); else env group `group` (xr_batch_step_group), its slot lo at row 0 of out_dev.
// out_u8 != null: the uint8 observation into out_u8 (xr_batch_step_observe_u8; out_dev unused, env_stride in bytes)
int32_t step_observe_impl(xr_batch* b, const int32_t* actions_dev, float* out_dev, int64_t env_stride, void* stream, bool inplace, int group = -1,
                          uint8_t* out_u8 = nullptr);

// uint8 observation buffers: 16-byte aligned rows of env_stride bytes (a multiple of 16), each at least (2+7 k_max) n_max long; every
// net id of every loaded region must fit a byte
int32_t u8_check(const xr_batch* b, const uint8_t* out, int64_t env_stride, const char* fn) {
    if ((reinterpret_cast<uintptr_t>(out) & 15) != 0 || env_stride % 16 != 0)
        return fail(XR_ERR_INVALID, "%s: out_dev must be 16-byte aligned and env_stride (bytes) a multiple of 16, got %p / %lld", fn,
                    static_cast<const void*>(out), (long long)env_stride);
    if (env_stride < full_row(b))
        return fail(XR_ERR_RANGE, "%s: env_stride %lld < (2+7*k_max)*n_max = %lld bytes", fn, (long long)env_stride, (long long)full_row(b));
    if (b->k_max > 255)
        return fail(XR_ERR_RANGE, "%s: a loaded region has %d nets; a uint8 observation holds net ids up to 255", fn, b->k_max);
    return XR_OK;
}
}

int32_t xr_batch_step_observe(xr_batch* b, const int32_t* actions_dev, float* out_dev, int64_t env_stride, void* stream) {
    return step_observe_impl(b, actions_dev, out_dev, env_stride, stream, false);
}

int32_t xr_batch_step_observe_inplace(xr_batch* b, const int32_t* actions_dev, float* out_dev, int64_t env_stride, void* stream) {
    return step_observe_impl(b, actions_dev, out_dev, env_stride, stream, true);
}

namespace {
int32_t step_observe_impl(xr_batch* b, const int32_t* actions_dev, float* out_dev, int64_t env_stride, void* stream, bool inplace, int group,
                          uint8_t* out_u8) {
    const bool u8 = out_u8 != nullptr;
    if (!b || !actions_dev || (!out_dev && !u8)) return fail(XR_ERR_INVALID, "xr_batch_step_observe: null argument");
    if (!b->loaded) return fail(XR_ERR_STATE, "xr_batch_step_observe: load regions first");
    if (u8) {
        if (const int32_t rc = u8_check(b, out_u8, env_stride, "xr_batch_step_observe_u8")) return rc;
    } else if (env_stride < full_row(b)) {
        return fail(XR_ERR_RANGE, "xr_batch_step_observe: env_stride %lld < (2+7*k_max)*n_max = %lld", (long long)env_stride, (long long)full_row(b));
    }
    XR_HIP(hipSetDevice(b->cfg.device));
    XrBatchDev d = b->dev;
    // the slots of this call: [lo, lo + n).  Every host decision below that a batch takes by its size takes the call's size.
    const int lo = group < 0 ? 0 : group_view(b, group, d);
    const int n = group < 0 ? b->cfg.n_envs : d.env_count;
    // in-place bookkeeping of this call: the batch-wide buffer, or the group's own
    ObsValid& valid = group < 0 ? b->obs_valid : b->group_valid[group];
    const void* const out_key = u8 ? static_cast<const void*>(out_u8) : static_cast<const void*>(out_dev);
    // in-place for this call: only when THIS buffer holds the observation of the state before the step (else: a full write)
    const bool inc = inplace && valid.holds(out_key, env_stride, u8);
    // which router runs the route tasks of a queue-form launch (auto: sweeps for the full rewrite of a large batch, see load; a group
    // takes them only when it is that large itself)
    const bool use_sweep = b->sweep_full && !inc && n >= 4096;
    const XrRouteVariant qv = route_variant(b, use_sweep);
    if (u8) {
        // the uint8 form always runs the queue form: its limits, and the LDS of the unit writer for planes that are not 16-byte aligned,
        // are checked before anything changes
        if (b->cfg.n_envs > (1 << 18) || b->k_max >= (1 << 14) || b->k_max < 1)
            return fail(XR_ERR_RANGE, "xr_batch_step_observe_u8: the queue form needs 1 <= k_max < 16384 and n_envs <= 262144 (k_max %d, n_envs %d)",
                        b->k_max, b->cfg.n_envs);
        if (!b->all_n_mult16) {
            const size_t need = ((size_t)(b->n_max + 15) / 16 + 2) * 4;
            if (need > qv.lds_bytes)
                return fail(XR_ERR_RANGE, "xr_batch_step_observe_u8: regions with N %% 16 != 0 need %zu bytes of LDS for the unit writer's masks, the step "
                            "kernel has %zu", need, qv.lds_bytes);
        }
    }
    if (group < 0) {
        for (ObsValid& v : b->group_valid) v.clear();      // every slot's state changes
    } else {
        b->obs_valid.clear();                       // the batch-wide buffer no longer holds this group's state
        actions_dev = shift_back(actions_dev, lo);
    }
    if (u8) d.obs_out_u8 = shift_back(out_u8, (int64_t)lo * env_stride);
    else d.obs_out = shift_back(out_dev, (int64_t)lo * env_stride);
    d.obs_stride = env_stride;
    d.obs_vec4 = u8 ? (b->all_n_mult16 ? 1 : 2)          // (uint8: 1 = every N % 16 == 0, 2 = LDS-mask writer)
                    : obs_store_mode(b, out_dev, env_stride);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool can_split = (d.obs_vec4 == 1 || (d.obs_vec4 == 2 && b->n_max <= 60 * 1024)) && b->cfg.n_envs <= (1 << 18) && b->k_max < (1 << 14) && b->k_max >= 1;
    const bool split = can_split && b->cfg.obs_mode == XR_OBS_SPLIT && !b->cfg.stream_per_region;
    // (uint8: always the queue form — obs_mode, obs_helper_blocks and stream_per_region do not apply)
    if (u8 || (can_split && (b->cfg.obs_mode == XR_OBS_QUEUE || b->cfg.obs_mode == 0) && !b->cfg.stream_per_region)) {      // the default: measured fastest
        // plan, then one persistent launch: as many workgroups as the chip holds (occupancy x CUs) drain the two queues
        b->last_obs_mode = XR_OBS_QUEUE;
        d.obs_head_only = 1;
        d.obs_split_pm = 1000;
        d.obs_incremental = inc ? 1 : 0;
        b->last_obs_inplace = d.obs_incremental;
        valid.clear();                              // (set again below once every launch of this call has been enqueued without error)
        d.queue_quota_pm = b->cfg.obs_split_permille > 0 ? b->cfg.obs_split_permille : 750;
        {
            // which workgroups start with units instead of a route: bit 5 of the workgroup index.  Bit 0 (rounds 1-2) put every
            // route-first workgroup on the even XCDs (workgroup i runs on XCD i % 8).  Same box, ms per step kernel, bit 0 -> 3 -> 5 ->
            // 8 -> none: 512 envs 0.296 -> 0.291 -> 0.290 -> 0.296 -> 0.302; 1024 envs 0.500 -> 0.489 -> 0.487 -> 0.485 -> 0.525;
            // 4096 envs 1.741 -> 1.736 -> 1.730 -> 1.733 -> 1.797 (profiles/r03_r_ab_queue_unit_first_workgroups.txt)
            static const int skip_env = [] { const char* v = getenv("XR_QUEUE_SKIP_SHIFT"); return v ? atoi(v) : -2; }();      // experiments only
            d.queue_skip_shift = skip_env != -2 ? skip_env : 5;
        }
        if (b->n_cus == 0) {            // once per batch: CUs x resident workgroups per CU of the step kernel (both variants)
            hipDeviceProp_t prop;
            XR_HIP(hipGetDeviceProperties(&prop, b->cfg.device));
            int per_cu = 0;
            size_t stat = 0;
            XR_HIP(xr_route_occupancy(route_variant(b), &per_cu, &stat));
            b->n_cus = prop.multiProcessorCount;
            b->queue_blocks = std::max(1, per_cu) * b->n_cus;
            if (b->sweep_full) {
                XR_HIP(xr_route_occupancy(route_variant(b, true), &per_cu, &stat));
                b->queue_blocks_sweep = std::max(1, per_cu) * b->n_cus;
            }
        }
        // this call's counters / the other bank (zeroed by this call's plan for the next one: no memset per call).  An env group has two
        // banks of its own, and its units their own slice of plan_units (at most k_max per env): group launches share no queue state
        int& bank = group < 0 ? b->queue_bank : b->group_bank[group];
        uint32_t* const banks = group < 0 ? b->queue.p : b->group_queue.p + 8 * group;
        d.queue = banks + 4 * bank;
        uint32_t* const next_queue = banks + 4 * (bank ^ 1);
        bank ^= 1;
        b->queue_last = d.queue;
        if (group >= 0) {
            d.plan_units = b->plan_units.p + (size_t)lo * std::max(1, b->k_max);
            d.plan_unit_net = b->plan_unit_net.p + (size_t)lo * std::max(1, b->k_max);
        }
        // Route tasks: slot order for large batches (longest-first measured SLOWER there, full rewrite 1.72 -> 1.83 ms, in-place
        // 1.06 -> 1.09 ms — the launch is bound by its write stream, and long routes up front delay the first units).  A batch of at
        // most ~2 routes per resident workgroup is different: its launch ends with the longest route, and a workgroup that starts
        // with units takes its route ~125 us late (tools/queue_timeline_probe.py, 1024 envs: the last route ends at 100 % of the
        // launch) — there the tasks are handed out longest predicted route first (xr_route_order_kernel, ~10 us).
        // Measured (profiles/r03_o_ab_queue_task_order.txt, same box, ms per step, slot order -> longest first): synthetic regions 512 /
        // 1024 / 2048 / 4096 envs 0.324 / 0.518 / 0.939 / 1.749 -> 0.318 / 0.513 / 0.945 / 1.849; the regions extracted from ispd18_test1
        // (heavier, more varied routes: their step is bound by routing) 1024 / 2048 / 4096 / 8192 slots 1.097 / 1.391 / 2.071 / 3.556 ->
        // 0.931 / 1.023 / 1.951 / 3.829.  Hence: up to 2 routes per resident workgroup, 4 for regions with unaligned planes.
        const int lpt_limit = (b->all_n_mult4 ? 2 : 4) * b->queue_blocks;
        const bool lpt_tasks = b->cfg.launch_order == 2 ||
                               (b->cfg.launch_order == 0 && b->queue_blocks > 0 && n <= lpt_limit && n > 64);
        int order_done = 0;       // (a batch of <= 1024 envs: plan and order are ONE launch; every dependent dispatch costs a small batch ~8 us)
        int32_t* const order = b->route_order.p + lo;       // (a group's longest-first order: its own slice)
        XR_HIP(xr_launch_plan(&d, actions_dev, next_queue, lpt_tasks ? order : nullptr, &order_done, st));
        if (lpt_tasks) {
            if (!order_done) XR_HIP(xr_launch_route_order(&d, actions_dev, order, st));
            d.route_order = order;
        }
        b->last_obs_sweeps = use_sweep ? 1 : 0;
        d.obs_lds_bytes = (int32_t)std::min<size_t>(qv.lds_bytes, 1u << 30);
        const int blocks = b->cfg.obs_writer_blocks > 0 ? b->cfg.obs_writer_blocks : (use_sweep ? b->queue_blocks_sweep : b->queue_blocks);
        // helper writers (aligned planes only): LDS-free workgroups on the internal stream draining the same unit queue;
        // forked after the plan, joined before the call returns the stream (events, no host wait)
        // (an env group runs without them: the internal stream and its events are the batch's, and group steps may run concurrently)
        const int helpers = !u8 && d.obs_vec4 == 1 && b->cfg.obs_helper_blocks > 0 ? b->cfg.obs_helper_blocks : 0;
        const bool use_helpers = helpers > 0 && n >= 64 && group < 0;
        if (use_helpers) {
            XR_HIP(hipEventRecord(b->ev_fork, st));
            XR_HIP(hipStreamWaitEvent(b->aux_stream, b->ev_fork, 0));
        }
        d.queue_grid = std::min(blocks, 4 * n);
        d.queue_slab_tickets = use_helpers ? 0 : 1;       // (the helpers take whole units from the same counter)
        XR_HIP(xr_launch_step_queue(&d, actions_dev, qv, d.queue_grid, st));
        if (use_helpers) {
            XR_HIP(xr_launch_unit_helpers(&d, helpers, b->aux_stream));
            XR_HIP(hipEventRecord(b->ev_join, b->aux_stream));
            XR_HIP(hipStreamWaitEvent(st, b->ev_join, 0));
        }
        valid.set(out_key, env_stride, u8);
        return XR_OK;
    }
    // (an env group takes the fused form where the batch would split: the split form's writer stream and events are the batch's)
    const bool split_here = split && group < 0;
    b->last_obs_mode = split_here ? XR_OBS_SPLIT : XR_OBS_FUSED;
    b->last_obs_inplace = 0;                                  // the fused and split forms always write the whole observation
    valid.clear();
    if (!split_here) {
        const int32_t rc = launch_route_form(b, d, actions_dev, st);
        if (rc == XR_OK) valid.set(out_dev, env_stride, false);
        return rc;
    }
    // plan (caller's stream) -> fork: net-plane writer on the internal stream || route kernel (+ planes 0..1) on the
    // caller's stream -> join.  Everything is ordered by events; the host never waits.
    d.obs_head_only = 1;
    d.obs_split_pm = b->cfg.obs_split_permille > 0 ? b->cfg.obs_split_permille : 1000;
    d.queue = b->queue.p + 4 * b->queue_bank;
    XR_HIP(xr_launch_plan(&d, actions_dev, b->queue.p + 4 * (b->queue_bank ^ 1), nullptr, nullptr, st));
    b->queue_bank ^= 1;
    b->queue_last = d.queue;
    XR_HIP(hipEventRecord(b->ev_fork, st));
    XR_HIP(hipStreamWaitEvent(b->aux_stream, b->ev_fork, 0));
    XR_HIP(xr_launch_route(&d, actions_dev, route_variant(b), st));
    XR_HIP(hipEventRecord(b->ev_w0, b->aux_stream));
    XR_HIP(xr_launch_netplanes(&d, b->cfg.obs_writer_blocks > 0 ? b->cfg.obs_writer_blocks : 512, d.obs_vec4 == 1 ? 1 : 0,
                               b->aux_stream));
    XR_HIP(hipEventRecord(b->ev_w1, b->aux_stream));
    XR_HIP(hipStreamWaitEvent(st, b->ev_w1, 0));
    valid.set(out_dev, env_stride, false);
    return XR_OK;
}
}  // namespace

int32_t xr_batch_step_compact(xr_batch* b, const int32_t* actions_dev, float* head_out_dev, int64_t head_stride, void* stream) {
    if (!b || !actions_dev || !head_out_dev) return fail(XR_ERR_INVALID, "xr_batch_step_compact: null argument");
    if (!b->loaded) return fail(XR_ERR_STATE, "xr_batch_step_compact: load regions first");
    if (head_stride < (int64_t)2 * b->n_max_nodes)
        return fail(XR_ERR_RANGE, "xr_batch_step_compact: head_stride %lld < 2*n_max = %lld", (long long)head_stride,
                    (long long)2 * b->n_max_nodes);
    XR_HIP(hipSetDevice(b->cfg.device));
    XrBatchDev d = b->dev;
    d.obs_out = head_out_dev;
    d.obs_stride = head_stride;
    d.obs_vec4 = obs_store_mode(b, head_out_dev, head_stride);
    if (d.obs_vec4 == 0)        // (the scalar epilogue has no head-only form)
        return fail(XR_ERR_INVALID, "xr_batch_step_compact: head_out_dev must be 16-byte aligned and head_stride a multiple of 4");
    drop_obs_valid(b);
    d.obs_head_only = 1;          // the epilogue writes planes 0..1 and the net planes of the lowest XR_SPLIT_KEEP ranks: none
    d.obs_split_pm = 1000;
    b->last_obs_mode = XR_OBS_FUSED;
    return launch_route_form(b, d, actions_dev, static_cast<hipStream_t>(stream));
}

int32_t xr_batch_net_planes(xr_batch* b, const int32_t* pair_region_dev, const int32_t* pair_net_dev, int32_t n_pairs,
                            float* out_dev, int64_t pair_stride, void* stream) {
    if (!b || !out_dev || (n_pairs > 0 && (!pair_region_dev || !pair_net_dev))) return fail(XR_ERR_INVALID, "xr_batch_net_planes: null argument");
    if (!b->loaded) return fail(XR_ERR_STATE, "xr_batch_net_planes: load regions first");
    if (n_pairs < 0 || pair_stride < (int64_t)7 * b->n_max_nodes)
        return fail(XR_ERR_RANGE, "xr_batch_net_planes: pair_stride %lld < 7*n_max = %lld", (long long)pair_stride,
                    (long long)7 * b->n_max_nodes);
    XR_HIP(hipSetDevice(b->cfg.device));
    const bool aligned = (pair_stride % 4 == 0) && ((reinterpret_cast<uintptr_t>(out_dev) & 15) == 0);
    XR_HIP(xr_launch_netplanes_pairs(&b->dev, pair_region_dev, pair_net_dev, n_pairs, out_dev, pair_stride, aligned ? 1 : 0,
                                     static_cast<hipStream_t>(stream)));
    return XR_OK;
}

namespace {
// bytes of a packed state row: the 16-byte head, the legal words, one bit per node of the largest region in 64-bit words
int64_t state_row_need(const xr_batch* b) { return 16 + 8 * ((int64_t)b->legal_words + ((b->n_max + 63) >> 6)); }

// The checks of the packed rows a caller hands to xr_batch_peek / xr_batch_tree_leaves.  They sit at two places of the check order, so
// there are two parts: ROWS_ALIGNED looks at no batch and comes before "load regions first", ROWS_LONG comes after the group check
enum RowPart { ROWS_ALIGNED, ROWS_LONG };
int32_t state_row_check(const xr_batch* b, const char* fn, const uint8_t* rows_out, int64_t row_bytes, RowPart part) {
    if (part == ROWS_ALIGNED) {
        if ((reinterpret_cast<uintptr_t>(rows_out) & 7) || row_bytes % 8 != 0)
            return fail(XR_ERR_INVALID, "%s: rows_out_dev %p / row_bytes %lld are not 8-byte aligned", fn, (const void*)rows_out, (long long)row_bytes);
        return XR_OK;
    }
    const int64_t need = state_row_need(b);
    if (row_bytes < need) return fail(XR_ERR_RANGE, "%s: row_bytes %lld < %lld (xr_batch_state_row_bytes)", fn, (long long)row_bytes, (long long)need);
    return XR_OK;
}
}  // namespace

int32_t xr_batch_state_row_bytes(const xr_batch* b, int64_t* row_bytes) {
    if (!b || !row_bytes) return fail(XR_ERR_INVALID, "xr_batch_state_row_bytes: null argument");
    if (!b->loaded) return fail(XR_ERR_STATE, "xr_batch_state_row_bytes: load regions first");
    *row_bytes = state_row_need(b);
    return XR_OK;
}

int32_t xr_batch_pack_state(xr_batch* b, uint8_t* rows_dev, int64_t row_bytes, int32_t region_base, void* stream) {
    if (!b || !rows_dev) return fail(XR_ERR_INVALID, "xr_batch_pack_state: null argument");
    if (!b->loaded) return fail(XR_ERR_STATE, "xr_batch_pack_state: load regions first");
    const int64_t need = state_row_need(b);
    if (row_bytes < need || row_bytes % 8 != 0 || (reinterpret_cast<uintptr_t>(rows_dev) & 7) != 0 || region_base < 0)
        return fail(XR_ERR_RANGE, "xr_batch_pack_state: row_bytes %lld (need >= %lld, a multiple of 8, 8-byte aligned rows), region_base %d",
                    (long long)row_bytes, (long long)need, region_base);
    XR_HIP(hipSetDevice(b->cfg.device));
    XR_HIP(xr_launch_pack_state(&b->dev, rows_dev, row_bytes, region_base, static_cast<hipStream_t>(stream)));
    return XR_OK;
}

int32_t xr_batch_expand_state(xr_batch* b, const uint8_t* rows_dev, int64_t row_bytes, int32_t n_rows, float* head_out_dev, int64_t head_stride,
                              int32_t* nlegal_out_dev, int32_t* region_out_dev, void* stream) {
    if (!b || (n_rows > 0 && (!rows_dev || !head_out_dev || !nlegal_out_dev || !region_out_dev)))
        return fail(XR_ERR_INVALID, "xr_batch_expand_state: null argument");
    if (!b->loaded) return fail(XR_ERR_STATE, "xr_batch_expand_state: load regions first");
    if (n_rows < 0 || row_bytes < 16 || row_bytes % 8 != 0 || (reinterpret_cast<uintptr_t>(rows_dev) & 7) != 0 || head_stride < (int64_t)2 * b->n_max_nodes)
        return fail(XR_ERR_RANGE, "xr_batch_expand_state: n_rows %d, row_bytes %lld (a multiple of 8, 8-byte aligned rows), head_stride %lld < 2*n_max = %lld",
                    n_rows, (long long)row_bytes, (long long)head_stride, (long long)2 * b->n_max_nodes);
    XR_HIP(hipSetDevice(b->cfg.device));
    const bool aligned = (head_stride % 4 == 0) && ((reinterpret_cast<uintptr_t>(head_out_dev) & 15) == 0);
    XR_HIP(xr_launch_expand_state(&b->dev, rows_dev, row_bytes, n_rows, head_out_dev, head_stride, nlegal_out_dev, region_out_dev, aligned ? 1 : 0,
                                  static_cast<hipStream_t>(stream)));
    return XR_OK;
}

int32_t xr_batch_ingest_state(xr_batch* b, const int16_t* owner_dev, const uint64_t* legal_dev, const int32_t* cum_dev, void* stream) {
    if (!b || !owner_dev || !legal_dev || !cum_dev) return fail(XR_ERR_INVALID, "xr_batch_ingest_state: null argument");
    if (!b->loaded) return fail(XR_ERR_STATE, "xr_batch_ingest_state: load regions first");
    if ((reinterpret_cast<uintptr_t>(owner_dev) & 15) != 0 || (reinterpret_cast<uintptr_t>(legal_dev) & 7) != 0 || (reinterpret_cast<uintptr_t>(cum_dev) & 3) != 0)
        return fail(XR_ERR_INVALID, "xr_batch_ingest_state: owner rows must be 16-byte aligned, legal words 8-byte, metrics 4-byte");
    XR_HIP(hipSetDevice(b->cfg.device));
    drop_obs_valid(b);                                // whatever observation a caller holds no longer describes the batch
    XR_HIP(xr_launch_ingest_state(&b->dev, owner_dev, legal_dev, cum_dev, static_cast<hipStream_t>(stream)));
    return XR_OK;
}

int32_t xr_batch_net_vectors(xr_batch* b, const int32_t* pair_region_dev, const int32_t* pair_net_dev, int32_t n_pairs, int32_t D, int32_t H, int32_t W,
                             const float* weights_dev, const float* bg_dev, float* out_dev, int32_t* flags_dev, int32_t normalize, void* stream) {
    if (!b || !weights_dev || !bg_dev || (n_pairs > 0 && (!pair_region_dev || !pair_net_dev || !out_dev || !flags_dev)))
        return fail(XR_ERR_INVALID, "xr_batch_net_vectors: null argument");
    if (!b->loaded) return fail(XR_ERR_STATE, "xr_batch_net_vectors: load regions first");
    if (n_pairs < 0 || D < 1 || H < 1 || W < 1) return fail(XR_ERR_RANGE, "xr_batch_net_vectors: n_pairs %d, grid %dx%dx%d", n_pairs, D, H, W);
    XR_HIP(hipSetDevice(b->cfg.device));
    int32_t status = XR_OK;
    XR_HIP(xr_launch_net_tower(b->regions.p, b->net_csr.p, b->ap_feat.p, b->n_regions, pair_region_dev, pair_net_dev, n_pairs, D, H, W, weights_dev, bg_dev, out_dev,
                               flags_dev, normalize, static_cast<hipStream_t>(stream), &status));
    if (status != XR_OK) return fail(status, "xr_batch_net_vectors: the fused net tower does not take a %dx%dx%d grid (the caller keeps the framework path)", D, H, W);
    return XR_OK;
}

int32_t xr_batch_route_occupancy(xr_batch* b, int32_t* workgroups_per_cu, int64_t* lds_bytes_per_workgroup) {
    if (!b || !workgroups_per_cu || !lds_bytes_per_workgroup) return fail(XR_ERR_INVALID, "xr_batch_route_occupancy: null argument");
    if (!b->loaded) return fail(XR_ERR_STATE, "xr_batch_route_occupancy: load regions first");
    XR_HIP(hipSetDevice(b->cfg.device));
    int n = 0;
    size_t stat = 0;
    XR_HIP(xr_route_occupancy(route_variant(b), &n, &stat));
    *workgroups_per_cu = n;
    *lds_bytes_per_workgroup = (int64_t)(b->route_lds + stat);
    return XR_OK;
}

int32_t xr_batch_observe_timing(xr_batch* b, int32_t* mode_out, float* writer_ms) {
    if (!b || !mode_out || !writer_ms) return fail(XR_ERR_INVALID, "xr_batch_observe_timing: null argument");
    *mode_out = b->last_obs_mode + (b->last_obs_mode == XR_OBS_QUEUE && b->last_obs_inplace ? 16 : 0)     // bit 4: the in-place form ran
                + (b->last_obs_mode == XR_OBS_QUEUE && b->last_obs_sweeps ? 32 : 0);                // bit 5: auto router took the sweeps
    *writer_ms = 0.f;
    if (b->last_obs_mode == XR_OBS_SPLIT) {
        XR_HIP(hipSetDevice(b->cfg.device));
        XR_HIP(hipEventSynchronize(b->ev_w1));
        XR_HIP(hipEventElapsedTime(writer_ms, b->ev_w0, b->ev_w1));
    }
    return XR_OK;
}

int32_t xr_batch_route_order(xr_batch* b, const int32_t* orders_dev, int32_t stride, int32_t* net_stats_dev, void* stream) {
    if (!b || !orders_dev) return fail(XR_ERR_INVALID, "xr_batch_route_order: null argument");
    if (!b->loaded) return fail(XR_ERR_STATE, "xr_batch_route_order: load regions first");
    if (stride < b->k_max)
        return fail(XR_ERR_RANGE, "xr_batch_route_order: stride %d < k_max %d", stride, b->k_max);
    XR_HIP(hipSetDevice(b->cfg.device));
    drop_obs_valid(b);
    XR_HIP(xr_launch_order(&b->dev, orders_dev, stride, net_stats_dev, route_variant(b), static_cast<hipStream_t>(stream)));
    return XR_OK;
}

int32_t xr_batch_random_actions(xr_batch* b, int32_t* actions_dev, uint64_t seed, void* stream) {
    if (!b || !actions_dev) return fail(XR_ERR_INVALID, "xr_batch_random_actions: null argument");
    if (!b->loaded) return fail(XR_ERR_STATE, "xr_batch_random_actions: load regions first");
    XR_HIP(hipSetDevice(b->cfg.device));
    XR_HIP(xr_launch_random_actions(&b->dev, actions_dev, seed, static_cast<hipStream_t>(stream)));
    return XR_OK;
}

int32_t xr_batch_observation(xr_batch* b, float* out_dev, int64_t env_stride, int32_t env_lo, int32_t env_hi,
                             void* stream) {
    if (!b || !out_dev) return fail(XR_ERR_INVALID, "xr_batch_observation: null argument");
    if (!b->loaded) return fail(XR_ERR_STATE, "xr_batch_observation: load regions first");
    if (env_lo < 0 || env_hi > b->cfg.n_envs || env_lo > env_hi)
        return fail(XR_ERR_RANGE, "xr_batch_observation: env range [%d,%d) outside [0,%d)", env_lo, env_hi, b->cfg.n_envs);
    if (env_stride < (int64_t)2 * b->n_max_nodes)
        return fail(XR_ERR_RANGE, "xr_batch_observation: env_stride %lld too small", (long long)env_stride);
    XR_HIP(hipSetDevice(b->cfg.device));
    XR_HIP(xr_launch_obs(&b->dev, out_dev, env_stride, env_lo, env_hi, b->n_max_nodes, obs_store_mode(b, out_dev, env_stride),
                         static_cast<hipStream_t>(stream)));
    if (env_stride >= full_row(b)) mark_obs_valid(b, out_dev, env_stride, false, env_lo, env_hi);      // (a shorter row cannot hold every region's observation)
    return XR_OK;
}

int32_t xr_batch_observation_u8(xr_batch* b, uint8_t* out_dev, int64_t env_stride, int32_t env_lo, int32_t env_hi, void* stream) {
    if (!b || !out_dev) return fail(XR_ERR_INVALID, "xr_batch_observation_u8: null argument");
    if (!b->loaded) return fail(XR_ERR_STATE, "xr_batch_observation_u8: load regions first");
    if (env_lo < 0 || env_hi > b->cfg.n_envs || env_lo > env_hi)
        return fail(XR_ERR_RANGE, "xr_batch_observation_u8: env range [%d,%d) outside [0,%d)", env_lo, env_hi, b->cfg.n_envs);
    if (const int32_t rc = u8_check(b, out_dev, env_stride, "xr_batch_observation_u8")) return rc;
    XR_HIP(hipSetDevice(b->cfg.device));
    XrBatchDev d = b->dev;
    d.obs_out_u8 = out_dev;
    d.obs_stride = env_stride;
    XR_HIP(xr_launch_obs_u8(&d, out_dev, env_stride, env_lo, env_hi, b->n_max_nodes, b->k_max, static_cast<hipStream_t>(stream)));
    mark_obs_valid(b, out_dev, env_stride, true, env_lo, env_hi);
    return XR_OK;
}

namespace {
// One device array of the batch as the fetch / store entry points see it (selector XR_FETCH_*)
struct ArrayRef {
    void* p;
    size_t row;            // bytes per env slot; 0: one scalar for the whole batch
    size_t bytes;          // the whole array
    bool store, group;     // admitted by xr_batch_store (part of the env state) / by xr_batch_fetch_group (a per-env array a group may slice)
};

bool array_ref(const xr_batch* b, int32_t what, ArrayRef& a) {
    const bool S = true, G = true;      // admitted by xr_batch_store / by xr_batch_fetch_group (!S, !G: not)
    switch (what) {
    case XR_FETCH_CUM: a = {b->cum.p, 3 * sizeof(int32_t), 0, S, G}; break;
    case XR_FETCH_DELTA: a = {b->delta.p, 3 * sizeof(int32_t), 0, S, G}; break;
    case XR_FETCH_REWARD: a = {b->reward.p, sizeof(double), 0, S, G}; break;
    case XR_FETCH_DONE: a = {b->done.p, 1, 0, S, G}; break;
    case XR_FETCH_NLEGAL: a = {b->nlegal.p, sizeof(int32_t), 0, S, G}; break;
    case XR_FETCH_STATUS: a = {b->status.p, sizeof(int32_t), 0, S, G}; break;
    case XR_FETCH_LEGAL: a = {b->legal.p, (size_t)b->legal_words * sizeof(uint64_t), 0, S, G}; break;
    case XR_FETCH_PATH_LEN: a = {b->path_len.p, sizeof(int32_t), 0, S, G}; break;
    case XR_FETCH_PATH: a = {b->path.p, (size_t)b->path_cap * sizeof(int32_t), 0, !S, G}; break;
    case XR_FETCH_OWNER: a = {b->owner.p, (size_t)b->n_max * sizeof(int16_t), 0, S, G}; break;
    case XR_FETCH_HASH: a = {b->hash.p, sizeof(uint64_t), 0, S, G}; break;
    case XR_FETCH_REGION: a = {b->env_region.p, sizeof(int32_t), 0, S, G}; break;
    case XR_FETCH_STEPS: a = {b->total_steps.p, 0, sizeof(int64_t), S, !G}; break;
    case XR_FETCH_SWEEPS: a = {b->sweeps.p, sizeof(int32_t), 0, !S, G}; break;
    case XR_FETCH_UNITS: a = {(b->queue_last ? b->queue_last : b->queue.p) + 2, 0, sizeof(uint32_t), !S, !G}; break;
    case XR_FETCH_ROUTE_ORDER: a = {b->route_order.p, sizeof(int32_t), 0, !S, !G}; break;
    case XR_FETCH_TOUCHED: a = {b->touched.p, sizeof(int32_t), 0, !S, !G}; break;
    case XR_FETCH_RECORD: a = {b->records.p, sizeof(XrStepRecord), 0, S, G}; break;
    case XR_FETCH_PHASES: a = {b->phase_cycles.p, 8 * sizeof(long long), 0, !S, !G}; break;
    case XR_FETCH_REPLAY: a = {b->env_replay.p, sizeof(int32_t), 0, S, G}; break;
    case XR_FETCH_ENV_STEPS: a = {b->env_steps.p, sizeof(int64_t), 0, S, G}; break;
    default: return false;
    }
    if (a.row) a.bytes = (size_t)b->cfg.n_envs * a.row;
    return true;
}
}  // namespace

int32_t xr_batch_fetch(xr_batch* b, int32_t what, void* dst_dev, size_t dst_bytes, void* stream) {
    if (!b || !dst_dev) return fail(XR_ERR_INVALID, "xr_batch_fetch: null argument");
    if (!b->loaded) return fail(XR_ERR_STATE, "xr_batch_fetch: load regions first");
    ArrayRef a;
    if (!array_ref(b, what, a)) return fail(XR_ERR_INVALID, "xr_batch_fetch: unknown selector %d", what);
    const void* const src = a.p;
    const size_t bytes = a.bytes;
    if (dst_bytes < bytes)
        return fail(XR_ERR_RANGE, "xr_batch_fetch(%d): destination holds %zu bytes, need %zu", what, dst_bytes, bytes);
    XR_HIP(hipSetDevice(b->cfg.device));
    // (hipMemcpyDefault: the destination may be a device buffer or PINNED host memory — one copy straight to the host for
    // the small-batch path)
    XR_HIP(hipMemcpyAsync(dst_dev, src, bytes, hipMemcpyDefault, static_cast<hipStream_t>(stream)));
    return XR_OK;
}

int32_t xr_batch_store(xr_batch* b, int32_t what, const void* src_dev, size_t src_bytes, void* stream) {
    if (!b || !src_dev) return fail(XR_ERR_INVALID, "xr_batch_store: null argument");
    if (!b->loaded) return fail(XR_ERR_STATE, "xr_batch_store: load regions first");
    const size_t B = (size_t)b->cfg.n_envs;
    ArrayRef a;
    if (!array_ref(b, what, a) || !a.store) return fail(XR_ERR_INVALID, "xr_batch_store: selector %d is not part of the env state", what);
    void* const dst = a.p;
    const size_t bytes = a.bytes;
    if (src_bytes != bytes)
        return fail(XR_ERR_RANGE, "xr_batch_store(%d): source holds %zu bytes, the array has %zu", what, src_bytes, bytes);
    XR_HIP(hipSetDevice(b->cfg.device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    // The arrays the kernels INDEX with are validated on the host before they reach the device (a restore is not a hot path: one small
    // staging copy + a stream sync): a region index outside the loaded regions, or legal bits / a nets-left count beyond the region's
    // nets, would make the next plan / route kernel read regions[], net_csr[] and net_work[] out of bounds — a device fault, not XR_ERR_RANGE.
    // Restore order for a consistent check: XR_FETCH_REGION before XR_FETCH_LEGAL / XR_FETCH_NLEGAL (RegionBatch.load_state_dict does).
    if (what == XR_FETCH_REGION || what == XR_FETCH_LEGAL || what == XR_FETCH_NLEGAL) {
        std::vector<unsigned char> host(bytes);
        std::vector<int32_t> reg(B);
        XR_HIP(hipMemcpyAsync(host.data(), src_dev, bytes, hipMemcpyDefault, st));
        if (what != XR_FETCH_REGION) XR_HIP(hipMemcpyAsync(reg.data(), b->env_region.p, B * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        XR_HIP(hipStreamSynchronize(st));
        if (what == XR_FETCH_REGION) {
            const int32_t* r = reinterpret_cast<const int32_t*>(host.data());
            for (size_t e = 0; e < B; e++)
                if (r[e] < 0 || r[e] >= b->n_regions)
                    return fail(XR_ERR_RANGE, "xr_batch_store(region): env %zu -> region %d outside 0..%d", e, r[e], b->n_regions - 1);
        } else if (what == XR_FETCH_NLEGAL) {
            const int32_t* nl = reinterpret_cast<const int32_t*>(host.data());
            for (size_t e = 0; e < B; e++)
                if (nl[e] < 0 || nl[e] > b->h_n_nets[reg[e]])
                    return fail(XR_ERR_RANGE, "xr_batch_store(nlegal): env %zu: %d nets left, its region %d has %d", e, nl[e], reg[e], b->h_n_nets[reg[e]]);
        } else {
            const uint64_t* lg = reinterpret_cast<const uint64_t*>(host.data());
            for (size_t e = 0; e < B; e++) {
                const int K = b->h_n_nets[reg[e]];
                for (int w = 0; w < b->legal_words; w++) {
                    const int lo = w * 64;
                    const uint64_t allowed = K >= lo + 64 ? ~0ULL : (K > lo ? ((1ULL << (K - lo)) - 1ULL) : 0ULL);
                    if (lg[e * b->legal_words + w] & ~allowed)
                        return fail(XR_ERR_RANGE, "xr_batch_store(legal): env %zu: net bits beyond the %d nets of its region %d", e, K, reg[e]);
                }
            }
        }
    }
    drop_obs_valid(b);                                // whatever observation a caller holds no longer describes the batch
    XR_HIP(hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDefault, st));
    return XR_OK;
}

// ---- env groups ----------------------------------------------------------------------------------------------------------------
// Audit of what a group step shares with the rest of the batch (xr_batch_step_group may run on several streams at once):
//   per-env rows (owner, legal, cum, hash, env_steps, replay, region, records, router scratch, plan_region): a group touches its own only;
//   plan_units / plan_unit_net: B*k_max entries, a group's units go to its slice at lo*k_max (at most k_max per env); route_order: the
//     group's slice at lo; queue counters: two banks per group (group_queue), the plan of group g zeroes only g's next bank;
//   total_steps: a device atomic; net_meas: racy per (region, net) bytes that steer launch orders only — no result depends on them;
//   aux_stream, ev_fork / ev_join, ev_w0 / ev_w1: the batch's — a group step never uses the helper writers or the split form (it runs the
//     fused form instead, same bytes); stream_per_region: the slot launches of the group's envs only, forked from and joined to the
//     caller's stream (the pool's events are re-recorded per call; host calls are serialised);
//   queue_last / last_obs_mode / last_obs_inplace: what the last call on the batch did.
// No workgroup of the persistent step-queue launch ever waits for another one (tasks are claimed by atomics; a workgroup's static first
// task just runs whenever it is scheduled), so several such launches sized for the whole chip may share it in any interleaving.

int32_t xr_batch_set_groups(xr_batch* b, const int32_t* bounds_host, int32_t n_groups) {
    if (!b || !bounds_host) return fail(XR_ERR_INVALID, "xr_batch_set_groups: null argument");
    if (n_groups < 1 || n_groups > XR_MAX_GROUPS || n_groups > b->cfg.n_envs)
        return fail(XR_ERR_RANGE, "xr_batch_set_groups: n_groups %d outside 1..min(%d, n_envs = %d)", n_groups, XR_MAX_GROUPS, b->cfg.n_envs);
    if (bounds_host[0] != 0 || bounds_host[n_groups] != b->cfg.n_envs)
        return fail(XR_ERR_INVALID, "xr_batch_set_groups: bounds must run from 0 to n_envs = %d (got %d .. %d)", b->cfg.n_envs, bounds_host[0],
                    bounds_host[n_groups]);
    for (int g = 0; g < n_groups; g++)
        if (bounds_host[g + 1] <= bounds_host[g])
            return fail(XR_ERR_INVALID, "xr_batch_set_groups: bounds not strictly ascending at group %d (%d, %d): no group may be empty", g,
                        bounds_host[g], bounds_host[g + 1]);
    XR_HIP(hipSetDevice(b->cfg.device));
    if (b->group_queue.p) XR_HIP(hipMemset(b->group_queue.p, 0, (size_t)XR_MAX_GROUPS * 8 * sizeof(uint32_t)));
    b->n_groups = n_groups;
    for (int g = 0; g <= n_groups; g++) b->group_bounds[g] = bounds_host[g];
    for (int g = 0; g < XR_MAX_GROUPS; g++) { b->group_bank[g] = 0; b->group_valid[g].clear(); }
    for (xr_batch::EvalPool& ep : b->eval) ep.keyed = false;          // a keyed tree belongs to the rows of the groups it was searched under
    return XR_OK;
}

namespace {
int32_t group_check(xr_batch* b, int32_t group, const char* fn) {
    if (!b->loaded) return fail(XR_ERR_STATE, "%s: load regions first", fn);
    if (group < 0 || group >= b->n_groups) return fail(XR_ERR_RANGE, "%s: group %d outside 0..%d", fn, group, b->n_groups - 1);
    return XR_OK;
}
}  // namespace

int32_t xr_batch_step_group(xr_batch* b, int32_t group, const int32_t* actions_dev, float* out_dev, int64_t env_stride, int32_t flags, void* stream) {
    if (!b || !actions_dev) return fail(XR_ERR_INVALID, "xr_batch_step_group: null argument");
    if (const int32_t rc = group_check(b, group, "xr_batch_step_group")) return rc;
    if (flags & ~XR_GROUP_INPLACE) return fail(XR_ERR_INVALID, "xr_batch_step_group: unknown flags 0x%x", flags);
    if (out_dev) return step_observe_impl(b, actions_dev, out_dev, env_stride, stream, (flags & XR_GROUP_INPLACE) != 0, group);
    XR_HIP(hipSetDevice(b->cfg.device));
    b->obs_valid.clear();
    b->group_valid[group].clear();
    XrBatchDev d = b->dev;
    const int lo = group_view(b, group, d);
    return launch_route_form(b, d, shift_back(actions_dev, lo), static_cast<hipStream_t>(stream));
}

int32_t xr_batch_step_observe_u8(xr_batch* b, int32_t group, const int32_t* actions_dev, uint8_t* out_dev, int64_t env_stride, int32_t flags,
                                 void* stream) {
    if (!b || !actions_dev || !out_dev) return fail(XR_ERR_INVALID, "xr_batch_step_observe_u8: null argument");
    if (flags & ~XR_OBS_U8_INPLACE) return fail(XR_ERR_INVALID, "xr_batch_step_observe_u8: unknown flags 0x%x", flags);
    if (group != -1)
        if (const int32_t rc = group_check(b, group, "xr_batch_step_observe_u8")) return rc;
    return step_observe_impl(b, actions_dev, nullptr, env_stride, stream, (flags & XR_OBS_U8_INPLACE) != 0, group, out_dev);
}

int32_t xr_batch_random_actions_group(xr_batch* b, int32_t group, int32_t* actions_dev, uint64_t seed, void* stream) {
    if (!b || !actions_dev) return fail(XR_ERR_INVALID, "xr_batch_random_actions_group: null argument");
    if (const int32_t rc = group_check(b, group, "xr_batch_random_actions_group")) return rc;
    XR_HIP(hipSetDevice(b->cfg.device));
    XrBatchDev d = b->dev;
    const int lo = group_view(b, group, d);
    XR_HIP(xr_launch_random_actions(&d, shift_back(actions_dev, lo), seed, static_cast<hipStream_t>(stream)));
    return XR_OK;
}

// group -1: the whole batch; else an env group, whose rows start at its first slot.  The kernel indexes the caller's rows from env_base
int32_t xr_batch_weighted_actions(xr_batch* b, int32_t group, const int32_t* weights_dev, int32_t k_cap, int32_t* actions_dev, uint64_t seed, void* stream) {
    if (!b || !weights_dev || !actions_dev) return fail(XR_ERR_INVALID, "xr_batch_weighted_actions: null argument");
    if (!b->loaded) return fail(XR_ERR_STATE, "xr_batch_weighted_actions: load regions first");
    if (group < -1 || group >= b->n_groups)
        return fail(XR_ERR_INVALID, "xr_batch_weighted_actions: group %d outside -1..%d", group, b->n_groups - 1);
    if (k_cap < b->k_max) return fail(XR_ERR_RANGE, "xr_batch_weighted_actions: k_cap %d < k_max %d", k_cap, b->k_max);
    if (!xr_launch_weighted_actions) return fail(XR_ERR_STATE, "xr_batch_weighted_actions: weighted sampling kernels not linked");
    XR_HIP(hipSetDevice(b->cfg.device));
    XrBatchDev d = b->dev;
    if (group >= 0) group_view(b, group, d);
    XR_HIP(xr_launch_weighted_actions(&d, weights_dev, k_cap, actions_dev, seed, static_cast<hipStream_t>(stream)));
    return XR_OK;
}

int32_t xr_batch_fetch_group(xr_batch* b, int32_t group, int32_t what, void* dst_dev, size_t dst_bytes, void* stream) {
    if (!b || !dst_dev) return fail(XR_ERR_INVALID, "xr_batch_fetch_group: null argument");
    if (const int32_t rc = group_check(b, group, "xr_batch_fetch_group")) return rc;
    ArrayRef a;
    if (!array_ref(b, what, a) || !a.group) return fail(XR_ERR_INVALID, "xr_batch_fetch_group: selector %d is not a per-env array", what);
    const char* const src = static_cast<const char*>(a.p);         // the array's row 0, and bytes per env row
    const size_t row = a.row;
    const int lo = b->group_bounds[group], n = b->group_bounds[group + 1] - lo;
    const size_t bytes = (size_t)n * row;
    if (dst_bytes != bytes)
        return fail(XR_ERR_RANGE, "xr_batch_fetch_group(%d): destination holds %zu bytes, the group's slice has %zu", what, dst_bytes, bytes);
    XR_HIP(hipSetDevice(b->cfg.device));
    XR_HIP(hipMemcpyAsync(dst_dev, src + (size_t)lo * row, bytes, hipMemcpyDefault, static_cast<hipStream_t>(stream)));
    return XR_OK;
}

// ---- lookahead -------------------------------------------------------------------------------------------------------------------
namespace {
// What the calls that take "group -1 (the whole batch) or an env group" share; every refusal names the entry point (fn).
// The caller's slots: [lo, lo + rows)
int32_t group_rows(const xr_batch* b, int32_t group, const char* fn, int& lo, int& rows) {
    if (group < -1 || group >= b->n_groups) return fail(XR_ERR_INVALID, "%s: group %d outside -1..%d", fn, group, b->n_groups - 1);
    lo = group < 0 ? 0 : b->group_bounds[group];
    rows = (group < 0 ? b->cfg.n_envs : b->group_bounds[group + 1]) - lo;
    return XR_OK;
}

// shadow slots route with the distance field in LDS, in one launch
int32_t lds_field_check(const xr_batch* b, const char* fn) {
    if (!b->lds_dist || b->cfg.stream_per_region)
        return fail(XR_ERR_RANGE, "%s: not available for batches whose distance field lives in HBM scratch (regions too large for LDS, "
                                  "force_scratch_field) or with stream_per_region", fn);
    return XR_OK;
}

// two alternating banks of `width` counters: this call's and the other one, which the next call takes
struct Banks { uint32_t *cur, *next; };
Banks flip_banks(uint32_t* ctr, int& bank, int width) {
    const Banks k{ctr + width * bank, ctr + width * (bank ^ 1)};
    bank ^= 1;
    return k;
}

// the shadow slots of a pool: look_grid slots of every state row, and the two rows of a launch that a router writes besides
size_t shadow_carve(const xr_batch* b, uint8_t* base, xr_batch::LookPool& lp) {
    const size_t G = (size_t)b->look_grid;
    Carver c;
    carve_slots(b, c, base, lp.rows, G);
    c.place(base, lp.total_steps, 1);
    c.place(base, lp.phase_cycles, G * 8);
    return c.off;
}

// once per load: CUs x resident workgroups per CU of the persistent lookahead kernel (the rollout kernel has its launch bounds and its
// dynamic LDS), at most one per possible (slot, net) pair
hipError_t look_grid_once(xr_batch* b, const XrRouteVariant& v) {
    if (b->look_grid != 0) return hipSuccess;
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, b->cfg.device);
    if (e != hipSuccess) return e;
    int per_cu = 0;
    e = xr_lookahead_occupancy(v, &per_cu);
    if (e != hipSuccess) return e;
    const int64_t pairs = (int64_t)b->cfg.n_envs * std::max(1, b->k_max);
    b->look_grid = (int)std::min<int64_t>((int64_t)std::max(1, per_cu) * prop.multiProcessorCount, pairs);
    return hipSuccess;
}

// the shadow view: the batch as it is configured NOW (guides may have been loaded since the pool was made), slot rows of the shadow slots
XrBatchDev shadow_view(const xr_batch* b, const xr_batch::LookPool& lp) {
    XrBatchDev sh = b->dev;
    copy_slot_rows(sh, lp.rows);
    sh.total_steps = lp.total_steps; sh.phase_cycles = lp.phase_cycles;
    sh.auto_reset = 0; sh.net_meas = nullptr; sh.obs_out = nullptr; sh.obs_out_u8 = nullptr; sh.route_order = nullptr;
    sh.n_envs = b->look_grid; sh.env_base = 0; sh.env_count = 0;
    return sh;
}

// The pool of one caller (whole batch / one env group), brought up on its first call: look_grid shadow slots in one allocation, a task list
// for every (slot, net) pair the batch can hold, two banks of counters; with roll_ctr, the claim counters of the rollout kernel too
int32_t shadow_pool(xr_batch* b, xr_batch::LookPool& lp, const XrRouteVariant& v, hipStream_t st, const char* fn, bool roll_ctr) {
    XR_HIP(look_grid_once(b, v));
    if (!lp.mem.p) {
        const size_t bytes = shadow_carve(b, nullptr, lp);
        hipError_t e = lp.mem.alloc(bytes);
        if (e == hipSuccess) e = lp.tasks.alloc((size_t)b->cfg.n_envs * std::max(1, b->k_max));
        if (e == hipSuccess) e = lp.ctr.alloc(4);
        if (e != hipSuccess) {
            lp.release();
            return fail(XR_ERR_NOMEM, "%s: hipMalloc of %zu bytes of shadow slots failed: %s", fn, bytes, hipGetErrorString(e));
        }
        if (hipMemsetAsync(lp.ctr.p, 0, 4 * sizeof(uint32_t), st) != hipSuccess ||          // both banks start clean; every plan zeroes the other bank
            hipMemsetAsync(lp.mem.p, 0, bytes, st) != hipSuccess) {
            lp.release();
            return fail(XR_ERR_HIP, "%s: clearing the shadow slots failed", fn);
        }
        shadow_carve(b, lp.mem.p, lp);
    }
    if (roll_ctr && !lp.roll_ctr.p) {          // both banks start clean; every launch zeroes the other bank
        if (lp.roll_ctr.alloc(2) != hipSuccess) return fail(XR_ERR_NOMEM, "%s: hipMalloc of the claim counters failed", fn);
        if (hipMemsetAsync(lp.roll_ctr.p, 0, 2 * sizeof(uint32_t), st) != hipSuccess) {
            lp.roll_ctr.release();
            return fail(XR_ERR_HIP, "%s: clearing the claim counters failed", fn);
        }
    }
    return XR_OK;
}

// What every call that plays in shadow slots starts from once its checks have passed: the caller's slots [lo, lo + rows), the stream, the
// router variant, the caller's pool and the shadow view of it
struct ShadowCall {
    int lo = 0, rows = 0;
    hipStream_t st = nullptr;
    XrRouteVariant v{};
    xr_batch::LookPool* lp = nullptr;
    XrBatchDev sh{};
};

// The one prologue: device, stream, variant, the pool of the caller (brought up on its first call; roll_ctr: with the claim counters of
// the line kernels), the view.  Allocates, so it comes after every check
int32_t shadow_call(xr_batch* b, int32_t group, int lo, int rows, void* stream, const char* fn, bool roll_ctr, ShadowCall& c) {
    XR_HIP(hipSetDevice(b->cfg.device));
    c.lo = lo; c.rows = rows;
    c.st = static_cast<hipStream_t>(stream);
    c.v = route_variant(b);
    c.lp = &b->look[group + 1];
    if (const int32_t rc = shadow_pool(b, *c.lp, c.v, c.st, fn, roll_ctr)) return rc;
    c.sh = shadow_view(b, *c.lp);
    return XR_OK;
}

// One line launch on the call's pool.  The caller has set l.kind, l.per_row and what is its own; everything the launches share is
// filled here: the views, the tasks (per_row lines for each of the caller's rows), this launch's claim counter (the banks flip), one
// workgroup per task up to the grid, and the two "absent means 0" rules — no prefix: stride 0, no order rows: k_cap 0
hipError_t launch_line(const xr_batch* b, const ShadowCall& c, XrLineLaunch l) {
    const int64_t tasks = (int64_t)c.rows * l.per_row;
    const Banks ctr = flip_banks(c.lp->roll_ctr.p, c.lp->roll_bank, 1);
    l.src = &b->dev; l.shadow = &c.sh; l.env_lo = c.lo; l.n_tasks = (int)tasks;
    l.ctr = ctr.cur; l.next_ctr = ctr.next;
    if (!l.prefix) l.prefix_stride = 0;
    if (!l.order_out) l.k_cap = 0;
    l.v = c.v; l.blocks = (int)std::min<int64_t>(b->look_grid, tasks);
    return xr_launch_line(&l, c.st);
}
}  // namespace

int32_t xr_batch_lookahead(xr_batch* b, int32_t group, const uint64_t* cand_mask_dev, int32_t* out_dev, int32_t k_cap, double* reward_out_dev,
                           void* stream) {
    if (!b || !out_dev) return fail(XR_ERR_INVALID, "xr_batch_lookahead: null argument");
    if (!b->loaded) return fail(XR_ERR_STATE, "xr_batch_lookahead: load regions first");
    int lo, rows;
    if (const int32_t rc = group_rows(b, group, "xr_batch_lookahead", lo, rows)) return rc;
    if (k_cap < b->k_max) return fail(XR_ERR_RANGE, "xr_batch_lookahead: k_cap %d < k_max %d", k_cap, b->k_max);
    if (const int32_t rc = lds_field_check(b, "xr_batch_lookahead")) return rc;
    if ((int64_t)b->cfg.n_envs * std::max(1, b->k_max) >= ((int64_t)1 << 31) || (int64_t)rows * k_cap >= ((int64_t)1 << 31))
        return fail(XR_ERR_RANGE, "xr_batch_lookahead: n_envs x k_max (or rows x k_cap) does not fit 31 bits");
    if (!xr_lookahead_occupancy || !xr_launch_lookahead_plan || !xr_launch_lookahead)
        return fail(XR_ERR_STATE, "xr_batch_lookahead: lookahead kernels not linked");
    ShadowCall c;
    if (const int32_t rc = shadow_call(b, group, lo, rows, stream, "xr_batch_lookahead", false, c)) return rc;
    const Banks ctr = flip_banks(c.lp->ctr.p, c.lp->bank, 2);          // its own banks, two counters wide: {tasks listed, next task}
    XR_HIP(xr_launch_lookahead_plan(&b->dev, lo, rows, cand_mask_dev, out_dev, reward_out_dev, k_cap, b->k_max, c.lp->tasks.p, ctr.cur, ctr.next, c.st));
    if (b->k_max < 1) return XR_OK;          // (no region has a net: the fill is the whole answer)
    const int blocks = (int)std::min<int64_t>(b->look_grid, (int64_t)rows * b->k_max);
    XR_HIP(xr_launch_lookahead(&b->dev, &c.sh, lo, c.lp->tasks.p, ctr.cur, out_dev, reward_out_dev, k_cap, b->k_max, c.v, blocks, c.st));
    return XR_OK;
}

// ---- rollouts ----------------------------------------------------------------------------------------------------------------------
namespace {
// xr_batch_rollout (weighted = false: policy 2 is unknown, the weights are not looked at) and xr_batch_rollout_weighted; every refusal
// names the entry point (fn)
int32_t rollout_impl(const char* fn, bool weighted, xr_batch* b, int32_t group, int32_t n_rollouts, int32_t policy, uint64_t seed, const int32_t* prefix_dev,
                     int32_t prefix_stride, int32_t max_plies, int32_t* out_dev, double* return_out_dev, uint64_t* hash_out_dev, int32_t* order_out_dev,
                     int32_t k_cap, const int32_t* weights_dev, int32_t weights_k_cap, void* stream) {
    if (!b || !out_dev) return fail(XR_ERR_INVALID, "%s: null argument", fn);
    if (!b->loaded) return fail(XR_ERR_STATE, "%s: load regions first", fn);
    int lo, rows;
    if (const int32_t rc = group_rows(b, group, fn, lo, rows)) return rc;
    const bool by_weights = weighted && policy == XR_ROLLOUT_WEIGHTED;
    if (policy != XR_ROLLOUT_STOP && policy != XR_ROLLOUT_RANDOM && !by_weights) return fail(XR_ERR_INVALID, "%s: unknown policy %d", fn, policy);
    if (by_weights && !weights_dev) return fail(XR_ERR_INVALID, "%s: null weights_dev with XR_ROLLOUT_WEIGHTED", fn);
    if (prefix_dev && prefix_stride < 1) return fail(XR_ERR_INVALID, "%s: prefix_stride %d < 1 with a prefix", fn, prefix_stride);
    if (max_plies < 0) return fail(XR_ERR_INVALID, "%s: max_plies %d is negative", fn, max_plies);
    if (n_rollouts < 1 || n_rollouts > XR_ROLLOUT_MAX)
        return fail(XR_ERR_RANGE, "%s: n_rollouts %d outside 1..%d", fn, n_rollouts, XR_ROLLOUT_MAX);
    if (order_out_dev && k_cap < b->k_max) return fail(XR_ERR_RANGE, "%s: k_cap %d < k_max %d", fn, k_cap, b->k_max);
    if (by_weights && weights_k_cap < b->k_max) return fail(XR_ERR_RANGE, "%s: weights_k_cap %d < k_max %d", fn, weights_k_cap, b->k_max);
    if (const int32_t rc = lds_field_check(b, fn)) return rc;
    const int64_t tasks = (int64_t)rows * n_rollouts;
    if (tasks >= ((int64_t)1 << 31)) return fail(XR_ERR_RANGE, "%s: rows x n_rollouts does not fit 31 bits", fn);
    if (!xr_lookahead_occupancy || !xr_launch_line) return fail(XR_ERR_STATE, "%s: rollout kernels not linked", fn);
    ShadowCall c;
    if (const int32_t rc = shadow_call(b, group, lo, rows, stream, fn, true, c)) return rc;
    XrLineLaunch l{};
    l.kind = by_weights ? XR_LINE_WEIGHTED : XR_LINE_POLICY; l.per_row = n_rollouts;
    l.policy = policy; l.seed = seed;
    l.prefix = prefix_dev; l.prefix_stride = prefix_stride; l.max_plies = max_plies;
    l.out = out_dev; l.return_out = return_out_dev; l.hash_out = hash_out_dev; l.order_out = order_out_dev; l.k_cap = k_cap;
    l.weights = weights_dev; l.weights_k_cap = weights_k_cap;
    XR_HIP(launch_line(b, c, l));
    return XR_OK;
}
}  // namespace

int32_t xr_batch_rollout(xr_batch* b, int32_t group, int32_t n_rollouts, int32_t policy, uint64_t seed, const int32_t* prefix_dev, int32_t prefix_stride,
                         int32_t max_plies, int32_t* out_dev, double* return_out_dev, uint64_t* hash_out_dev, int32_t* order_out_dev, int32_t k_cap,
                         void* stream) {
    return rollout_impl("xr_batch_rollout", false, b, group, n_rollouts, policy, seed, prefix_dev, prefix_stride, max_plies, out_dev, return_out_dev, hash_out_dev,
                        order_out_dev, k_cap, nullptr, 0, stream);
}

int32_t xr_batch_rollout_weighted(xr_batch* b, int32_t group, int32_t n_rollouts, int32_t policy, uint64_t seed, const int32_t* prefix_dev,
                                  int32_t prefix_stride, int32_t max_plies, int32_t* out_dev, double* return_out_dev, uint64_t* hash_out_dev,
                                  int32_t* order_out_dev, int32_t k_cap, const int32_t* weights_dev, int32_t weights_k_cap, void* stream) {
    return rollout_impl("xr_batch_rollout_weighted", true, b, group, n_rollouts, policy, seed, prefix_dev, prefix_stride, max_plies, out_dev, return_out_dev,
                        hash_out_dev, order_out_dev, k_cap, weights_dev, weights_k_cap, stream);
}

// ---- peek --------------------------------------------------------------------------------------------------------------------------
// xr_batch_rollout's checks in xr_batch_rollout's order, with the row arguments where the policy's were; the pool and the claim counters
// are the rollout's (calls on one pool are ordered by the caller)
int32_t xr_batch_peek(xr_batch* b, int32_t group, int32_t n_lines, const int32_t* prefix_dev, int32_t prefix_stride, int32_t max_plies,
                      uint8_t* rows_out_dev, int64_t row_bytes, int32_t region_base, int32_t* out_dev, double* return_out_dev, uint64_t* hash_out_dev,
                      int32_t* order_out_dev, int32_t k_cap, void* stream) {
    const char* fn = "xr_batch_peek";
    if (!b || !rows_out_dev || !out_dev) return fail(XR_ERR_INVALID, "%s: null argument", fn);
    if (const int32_t rc = state_row_check(b, fn, rows_out_dev, row_bytes, ROWS_ALIGNED)) return rc;
    if (!b->loaded) return fail(XR_ERR_STATE, "%s: load regions first", fn);
    int lo, rows;
    if (const int32_t rc = group_rows(b, group, fn, lo, rows)) return rc;
    if (prefix_dev && prefix_stride < 1) return fail(XR_ERR_INVALID, "%s: prefix_stride %d < 1 with a prefix", fn, prefix_stride);
    if (max_plies < 0) return fail(XR_ERR_INVALID, "%s: max_plies %d is negative", fn, max_plies);
    if (n_lines < 1 || n_lines > XR_PEEK_MAX) return fail(XR_ERR_RANGE, "%s: n_lines %d outside 1..%d", fn, n_lines, XR_PEEK_MAX);
    if (const int32_t rc = state_row_check(b, fn, rows_out_dev, row_bytes, ROWS_LONG)) return rc;
    if (order_out_dev && k_cap < b->k_max) return fail(XR_ERR_RANGE, "%s: k_cap %d < k_max %d", fn, k_cap, b->k_max);
    if (const int32_t rc = lds_field_check(b, fn)) return rc;
    if ((int64_t)rows * n_lines >= ((int64_t)1 << 31)) return fail(XR_ERR_RANGE, "%s: rows x n_lines does not fit 31 bits", fn);
    if (!xr_lookahead_occupancy || !xr_launch_line) return fail(XR_ERR_STATE, "%s: peek kernels not linked", fn);
    ShadowCall c;
    if (const int32_t rc = shadow_call(b, group, lo, rows, stream, fn, true, c)) return rc;
    XrLineLaunch l{};
    l.kind = XR_LINE_PEEK; l.per_row = n_lines;
    l.prefix = prefix_dev; l.prefix_stride = prefix_stride; l.max_plies = max_plies;
    l.rows = rows_out_dev; l.row_bytes = row_bytes; l.region_base = region_base;
    l.out = out_dev; l.return_out = return_out_dev; l.hash_out = hash_out_dev; l.order_out = order_out_dev; l.k_cap = k_cap;
    XR_HIP(launch_line(b, c, l));
    return XR_OK;
}

// ---- tree search -------------------------------------------------------------------------------------------------------------------
namespace {
bool tree_knobs_ok(double c_init, double c_base) { return std::isfinite(c_init) && std::isfinite(c_base) && c_base > 0.0; }

// E[n] of XR-Tree v1, one IEEE operation after the other
void tree_table_fill(double c_init, double c_base, int64_t from, int64_t to, double* out) {
    for (int64_t n = from; n <= to; n++) {
        const double x = ((double)n + c_base + 1.0) / c_base;
        out[n - from] = (std::log(x) + c_init) * std::sqrt((double)n);
    }
}
}  // namespace

int32_t xr_tree_exploration_table(double c_init, double c_base, int32_t n, double* out_host) {
    if (!out_host || n < 0) return fail(XR_ERR_INVALID, "xr_tree_exploration_table: null out_host or n %d < 0", n);
    if (!tree_knobs_ok(c_init, c_base)) return fail(XR_ERR_INVALID, "xr_tree_exploration_table: c_init must be finite and c_base finite and > 0");
    tree_table_fill(c_init, c_base, 0, n, out_host);
    return XR_OK;
}

namespace {
using TreeTables = std::vector<std::unique_ptr<xr_batch::TreeTable>>;

// Which uploaded table serves a call that wants E[0 .. e_max].  The searches take any table of their knobs that is long enough
// (TABLE_AT_LEAST: a later, longer call adds a table and the shorter one stays, since a launch in flight may read it); a session takes
// one of exactly its length (TABLE_EXACTLY: EvalPool keeps one per (c_init, c_base, max_sims)).  Both kernels clamp their index at the
// e_max they are handed, not at the table's length, so a longer table would serve a session as well; the rules stay as they were
enum TableMatch { TABLE_AT_LEAST, TABLE_EXACTLY };

// The exploration table of (c_init, c_base) among `tables`, found or built and uploaded: the single copy.  E: its device address
int32_t exploration_table(TreeTables& tables, double c_init, double c_base, int e_max, TableMatch match, hipStream_t st, const char* fn, const double*& E) {
    const size_t len = (size_t)e_max + 1;
    xr_batch::TreeTable* tab = nullptr;
    for (auto& t : tables)
        if (t->c_init == c_init && t->c_base == c_base && (match == TABLE_EXACTLY ? t->host.size() == len : t->host.size() >= len)) tab = t.get();
    if (!tab) {
        std::unique_ptr<xr_batch::TreeTable> t(new (std::nothrow) xr_batch::TreeTable);
        if (!t) return fail(XR_ERR_NOMEM, "%s: no host memory for the exploration table", fn);
        t->c_init = c_init; t->c_base = c_base;
        t->host.resize(len);
        tree_table_fill(c_init, c_base, 0, e_max, t->host.data());
        if (t->dev.alloc(t->host.size()) != hipSuccess) return fail(XR_ERR_NOMEM, "%s: hipMalloc of the exploration table failed", fn);
        XR_HIP(hipMemcpyAsync(t->dev.p, t->host.data(), t->host.size() * sizeof(double), hipMemcpyHostToDevice, st));
        tab = t.get();          // (the host copy stays: the asynchronous upload reads it)
        tables.push_back(std::move(t));
    }
    E = tab->dev.p;
    return XR_OK;
}

// What the three tree searches take: xr_batch_tree_search (sim_weights null, keep false), xr_batch_tree_search_weighted (Evaluate runs
// XR_ROLLOUT_WEIGHTED with the row's sim weights, [rows][k_cap], instead of XR_ROLLOUT_RANDOM) and xr_batch_tree_search_keep (keep: the
// same checks and the same waves on the caller's kept-tree pool, after xr_tree_keep_begin_kernel in place of the reset)
struct TreeSearchArgs {
    const char* fn = nullptr;          // the entry point: every refusal names it
    int32_t group = -1, n_waves = 0, n_par = 0, node_cap = 0, k_cap = 0;
    uint64_t seed = 0;
    double c_init = 0, c_base = 0;
    const float* prior = nullptr;
    const int32_t* sim_weights = nullptr;
    int32_t* visits_out = nullptr;
    double* value_out = nullptr;
    int32_t* info_out = nullptr;
    int32_t* best_order_out = nullptr;
    double* best_return_out = nullptr;
    int32_t* paths_out = nullptr;
    double* returns_out = nullptr;
    void* stream = nullptr;
    bool keep = false;
    const int32_t* played = nullptr;   // keep alone: null (every row is rebuilt), or [rows]
    int32_t* kept_out = nullptr;       // keep alone: null, or [rows][2]
};

// Step 1: every refusal, in the documented order, up to "do not fit any device".  Allocates nothing; k_cap leaves it at 1 or more
int32_t tree_check(const xr_batch* b, TreeSearchArgs& a, int& lo, int& rows) {
    const char* fn = a.fn;
    if (!b || !a.visits_out || !a.value_out || !a.info_out) return fail(XR_ERR_INVALID, "%s: null argument", fn);
    if (!b->loaded) return fail(XR_ERR_STATE, "%s: load regions first", fn);
    if (const int32_t rc = group_rows(b, a.group, fn, lo, rows)) return rc;
    if (a.n_waves < 1) return fail(XR_ERR_INVALID, "%s: n_waves %d < 1", fn, a.n_waves);
    if (a.n_par < 1) return fail(XR_ERR_INVALID, "%s: n_par %d < 1", fn, a.n_par);
    if (!std::isfinite(a.c_init)) return fail(XR_ERR_INVALID, "%s: c_init is not finite", fn);
    if (!tree_knobs_ok(a.c_init, a.c_base)) return fail(XR_ERR_INVALID, "%s: c_base must be finite and > 0", fn);
    if (a.n_par > XR_ROLLOUT_MAX) return fail(XR_ERR_RANGE, "%s: n_par %d above %d", fn, a.n_par, XR_ROLLOUT_MAX);
    if ((int64_t)a.n_waves * a.n_par > XR_TREE_MAX_SIMS)
        return fail(XR_ERR_RANGE, "%s: n_waves x n_par = %lld simulations above %d", fn, (long long)a.n_waves * a.n_par, XR_TREE_MAX_SIMS);
    if (a.node_cap < 1) return fail(XR_ERR_RANGE, "%s: node_cap %d < 1", fn, a.node_cap);
    if (a.k_cap < b->k_max) return fail(XR_ERR_RANGE, "%s: k_cap %d < k_max %d", fn, a.k_cap, b->k_max);
    if (const int32_t rc = lds_field_check(b, fn)) return rc;
    if ((int64_t)rows * a.n_par >= ((int64_t)1 << 31)) return fail(XR_ERR_RANGE, "%s: rows x n_par does not fit 31 bits", fn);
    if (!xr_lookahead_occupancy || !xr_launch_line || !xr_launch_tree_reset || !xr_launch_tree_select || !xr_launch_tree_backup ||
        (a.keep && !xr_launch_tree_keep_begin))
        return fail(XR_ERR_STATE, "%s: tree search kernels not linked", fn);
    if (a.k_cap < 1) a.k_cap = 1;
    if ((double)rows * ((a.keep ? 2.0 : 1.0) * (double)a.node_cap * sizeof(XrTreeNode) + (a.keep ? 8.0 * b->legal_words + 24.0 : 0.0) +
                        (double)a.n_par * (8.0 * a.k_cap + 40.0) + 64.0) > 1e15)
        return fail(XR_ERR_NOMEM, "%s: %d rows x %d nodes do not fit any device", fn, rows, a.node_cap);
    return XR_OK;
}

// Step 2: the private memory of the waves, grown to this call's shape — six arrays in one allocation, each starting on a 16-byte
// boundary (a kept call: four; its nodes and row states live in the kept pool).  rec: the rollout launch's records, read by no one
int32_t wave_memory(xr_batch* b, const TreeSearchArgs& a, int rows, XrTreeDev& t, int32_t*& rec) {
    Carver c;
    const size_t R = (size_t)rows, P = (size_t)a.n_par, K = (size_t)a.k_cap;
    const size_t o_nodes = a.keep ? 0 : c.take(R * (size_t)a.node_cap * sizeof(XrTreeNode)), o_rs = a.keep ? 0 : c.take(R * sizeof(XrTreeRow));
    const size_t o_prefix = c.take(R * P * K * sizeof(int32_t)), o_order = c.take(R * P * K * sizeof(int32_t));
    const size_t o_rec = c.take(R * P * 8 * sizeof(int32_t)), o_ret = c.take(R * P * sizeof(double));
    DevBuf<uint8_t>& mem = a.keep ? b->keep[a.group + 1].scratch : b->tree[a.group + 1].mem;
    if (mem.n < c.off && mem.alloc(c.off) != hipSuccess) {
        mem.release();
        return fail(XR_ERR_NOMEM, "%s: hipMalloc of %zu bytes of trees failed", a.fn, c.off);
    }
    uint8_t* const m = mem.p;
    if (!a.keep) { t.nodes = reinterpret_cast<XrTreeNode*>(m + o_nodes); t.rs = reinterpret_cast<XrTreeRow*>(m + o_rs); }
    t.prefix = reinterpret_cast<int32_t*>(m + o_prefix); t.order = reinterpret_cast<int32_t*>(m + o_order);
    t.ret = reinterpret_cast<double*>(m + o_ret);
    rec = reinterpret_cast<int32_t*>(m + o_rec);
    return XR_OK;
}

// the kept trees of a pool: two halves of nodes, the row states, the keys, their legal words
struct KeptCarve { size_t half[2], rs, key, legal, bytes; };
KeptCarve kept_carve(const xr_batch* b, int rows, int node_cap) {
    Carver c;
    const size_t R = (size_t)rows, half_bytes = R * (size_t)node_cap * sizeof(XrTreeNode);
    KeptCarve k{};
    k.half[0] = c.take(half_bytes); k.half[1] = c.take(half_bytes); k.rs = c.take(R * sizeof(XrTreeRow));
    k.key = c.take(R * sizeof(XrTreeKey)); k.legal = c.take(R * (size_t)b->legal_words * sizeof(uint64_t));
    k.bytes = c.off;
    return k;
}

// Step 3 (a kept call): the pool against this call's shape.  Another shape, or the first call: no row of the pool is a tree of this
// call's rows, every row is rebuilt and `played` is dropped; the pool grows if it has to.  From here until the first kernel is enqueued
// (kept_begin) the pool holds no trees
int32_t kept_pool(xr_batch* b, const TreeSearchArgs& a, int lo, int rows, bool& rebuild_all) {
    xr_batch::KeepPool& kp = b->keep[a.group + 1];
    const size_t bytes = kept_carve(b, rows, a.node_cap).bytes;
    rebuild_all = !a.played;
    if (kp.rows != rows || kp.lo != lo || kp.node_cap != a.node_cap || kp.k_cap != a.k_cap || kp.legal_words != b->legal_words || kp.trees.n < bytes) {
        rebuild_all = true;
        if (kp.trees.n < bytes && kp.trees.alloc(bytes) != hipSuccess) {
            kp.release();
            return fail(XR_ERR_NOMEM, "%s: hipMalloc of %zu bytes of kept trees failed", a.fn, bytes);
        }
    }
    kp.rows = 0;
    return XR_OK;
}

// Step 5 (a kept call), after the last step that can refuse, so that a refused call leaves the halves where they were: the half flip —
// this call searches in the other half and reads the last call's — and the first kernel, which re-roots or rebuilds every row
int32_t kept_begin(xr_batch* b, const TreeSearchArgs& a, int lo, int rows, bool rebuild_all, XrTreeDev& t, hipStream_t st) {
    xr_batch::KeepPool& kp = b->keep[a.group + 1];
    const KeptCarve k = kept_carve(b, rows, a.node_cap);
    uint8_t* const km = kp.trees.p;
    XrTreeKeepDev kd{};
    kd.old_nodes = reinterpret_cast<const XrTreeNode*>(km + k.half[kp.half]);
    kp.half ^= 1;
    t.nodes = reinterpret_cast<XrTreeNode*>(km + k.half[kp.half]); t.rs = reinterpret_cast<XrTreeRow*>(km + k.rs);
    kd.key = reinterpret_cast<XrTreeKey*>(km + k.key); kd.key_legal = reinterpret_cast<uint64_t*>(km + k.legal);
    kd.played = rebuild_all ? nullptr : a.played; kd.kept_out = a.kept_out; kd.n_add = t.n_sims;
    XR_HIP(xr_launch_tree_keep_begin(&b->dev, &t, &kd, rows, st));
    kp.rows = rows; kp.lo = lo; kp.node_cap = a.node_cap; kp.k_cap = a.k_cap; kp.legal_words = b->legal_words;
    return XR_OK;
}

// The last step: per wave select, the rollout launch of the wave's paths (its records go to rec, its returns and orders to the tree's
// rows), backup
int32_t run_waves(const xr_batch* b, const TreeSearchArgs& a, const ShadowCall& c, const XrTreeDev& t, int32_t* rec) {
    XrLineLaunch l{};
    l.kind = a.sim_weights ? XR_LINE_WEIGHTED : XR_LINE_POLICY; l.per_row = a.n_par;
    l.policy = XR_ROLLOUT_RANDOM;
    l.prefix = t.prefix; l.prefix_stride = a.k_cap;
    l.out = rec; l.return_out = t.ret; l.order_out = t.order; l.k_cap = a.k_cap;
    l.weights = a.sim_weights; l.weights_k_cap = a.k_cap;
    for (int w = 0; w < a.n_waves; w++) {
        XR_HIP(xr_launch_tree_select(&b->dev, &t, c.rows, w, c.st));
        l.seed = a.seed + (uint64_t)w * 0xD1B54A32D192ED03ULL;
        XR_HIP(launch_line(b, c, l));
        XR_HIP(xr_launch_tree_backup(&b->dev, &t, c.rows, w, w == a.n_waves - 1 ? 1 : 0, c.st));
    }
    return XR_OK;
}

int32_t tree_search_impl(xr_batch* b, TreeSearchArgs a) {
    int lo, rows;
    if (const int32_t rc = tree_check(b, a, lo, rows)) return rc;
    ShadowCall c;
    if (const int32_t rc = shadow_call(b, a.group, lo, rows, a.stream, a.fn, true, c)) return rc;
    XrTreeDev t{};
    int32_t* rec = nullptr;
    bool rebuild_all = false;
    if (const int32_t rc = wave_memory(b, a, rows, t, rec)) return rc;
    if (a.keep)
        if (const int32_t rc = kept_pool(b, a, lo, rows, rebuild_all)) return rc;
    t.n_sims = a.n_waves * a.n_par;
    t.e_max = a.keep ? XR_TREE_MAX_SIMS : t.n_sims;          // a kept root meets visit counts above this call's simulations
    if (const int32_t rc = exploration_table(a.keep ? b->keep[a.group + 1].tables : b->tree[a.group + 1].tables, a.c_init, a.c_base, t.e_max, TABLE_AT_LEAST, c.st,
                                             a.fn, t.E))
        return rc;
    t.prior = a.prior;
    t.node_cap = a.node_cap; t.n_par = a.n_par; t.k_cap = a.k_cap; t.env_lo = lo;
    t.visits_out = a.visits_out; t.value_out = a.value_out; t.info_out = a.info_out; t.best_order_out = a.best_order_out;
    t.best_return_out = a.best_return_out; t.paths_out = a.paths_out; t.returns_out = a.returns_out;
    if (a.keep) {
        if (const int32_t rc = kept_begin(b, a, lo, rows, rebuild_all, t, c.st)) return rc;
    } else {
        XR_HIP(xr_launch_tree_reset(&b->dev, &t, rows, c.st));
    }
    return run_waves(b, a, c, t, rec);
}

// what the three exports have in common, into `a` (by reference: this namespace lies inside extern "C")
void tree_args(TreeSearchArgs& a, const char* fn, int32_t group, int32_t n_waves, int32_t n_par, uint64_t seed, const float* prior_dev, int32_t node_cap, double c_init,
               double c_base, int32_t* visits_out_dev, double* value_out_dev, int32_t k_cap, int32_t* info_out_dev, int32_t* best_order_out_dev,
               double* best_return_out_dev, int32_t* paths_out_dev, double* returns_out_dev, void* stream) {
    a.fn = fn; a.group = group; a.n_waves = n_waves; a.n_par = n_par; a.seed = seed; a.prior = prior_dev; a.node_cap = node_cap;
    a.c_init = c_init; a.c_base = c_base; a.visits_out = visits_out_dev; a.value_out = value_out_dev; a.k_cap = k_cap; a.info_out = info_out_dev;
    a.best_order_out = best_order_out_dev; a.best_return_out = best_return_out_dev; a.paths_out = paths_out_dev; a.returns_out = returns_out_dev;
    a.stream = stream;
}
}  // namespace

int32_t xr_batch_tree_search(xr_batch* b, int32_t group, int32_t n_waves, int32_t n_par, uint64_t seed, const float* prior_dev, int32_t node_cap,
                             double c_init, double c_base, int32_t* visits_out_dev, double* value_out_dev, int32_t k_cap, int32_t* info_out_dev,
                             int32_t* best_order_out_dev, double* best_return_out_dev, int32_t* paths_out_dev, double* returns_out_dev, void* stream) {
    TreeSearchArgs a;
    tree_args(a, "xr_batch_tree_search", group, n_waves, n_par, seed, prior_dev, node_cap, c_init, c_base, visits_out_dev, value_out_dev, k_cap, info_out_dev,
              best_order_out_dev, best_return_out_dev, paths_out_dev, returns_out_dev, stream);
    return tree_search_impl(b, a);
}

int32_t xr_batch_tree_search_weighted(xr_batch* b, int32_t group, int32_t n_waves, int32_t n_par, uint64_t seed, const float* prior_dev, int32_t node_cap,
                                      double c_init, double c_base, int32_t* visits_out_dev, double* value_out_dev, int32_t k_cap, int32_t* info_out_dev,
                                      int32_t* best_order_out_dev, double* best_return_out_dev, int32_t* paths_out_dev, double* returns_out_dev,
                                      const int32_t* sim_weights_dev, void* stream) {
    TreeSearchArgs a;
    tree_args(a, "xr_batch_tree_search_weighted", group, n_waves, n_par, seed, prior_dev, node_cap, c_init, c_base, visits_out_dev, value_out_dev, k_cap, info_out_dev,
              best_order_out_dev, best_return_out_dev, paths_out_dev, returns_out_dev, stream);
    a.sim_weights = sim_weights_dev;
    return tree_search_impl(b, a);
}

int32_t xr_batch_tree_search_keep(xr_batch* b, int32_t group, const int32_t* played_dev, int32_t n_waves, int32_t n_par, uint64_t seed, const float* prior_dev,
                                  int32_t node_cap, double c_init, double c_base, int32_t* visits_out_dev, double* value_out_dev, int32_t k_cap,
                                  int32_t* info_out_dev, int32_t* best_order_out_dev, double* best_return_out_dev, int32_t* paths_out_dev,
                                  double* returns_out_dev, const int32_t* sim_weights_dev, int32_t* kept_out_dev, void* stream) {
    TreeSearchArgs a;
    tree_args(a, "xr_batch_tree_search_keep", group, n_waves, n_par, seed, prior_dev, node_cap, c_init, c_base, visits_out_dev, value_out_dev, k_cap, info_out_dev,
              best_order_out_dev, best_return_out_dev, paths_out_dev, returns_out_dev, stream);
    a.sim_weights = sim_weights_dev;
    a.keep = true; a.played = played_dev; a.kept_out = kept_out_dev;
    return tree_search_impl(b, a);
}

// ---- evaluated tree search ---------------------------------------------------------------------------------------------------------
// "XR-Tree v2, evaluated": open starts a session on the caller's pool, leaves runs one wave's select and its peek launch, backup takes
// the evaluator's values.  The host keeps the session's shape and its place in the call order; every refusal names its entry point.
// "XR-Tree v2, kept": reopen starts a keyed session that may continue from the trees the pool's last keyed session left
namespace {
// The pool of a session in one allocation, each array starting on a 16-byte boundary: xr_batch_tree_open's nine arrays, in its order; a
// keyed session's (xr_batch_tree_reopen) eleven — the second half of nodes after the first, the keys at the end
struct EvalCarve { size_t half[2], rs, prefix, ret, leaf, best, legal, nlegal, prior, key, bytes; };
EvalCarve eval_carve(const xr_batch* b, int rows, int n_par, int node_cap, int k_cap, bool keyed) {
    Carver c;
    const size_t R = (size_t)rows, P = (size_t)n_par, K = (size_t)k_cap, half_bytes = R * (size_t)node_cap * sizeof(XrTreeNode);
    EvalCarve v{};
    v.half[0] = c.take(half_bytes); v.half[1] = keyed ? c.take(half_bytes) : v.half[0]; v.rs = c.take(R * sizeof(XrTreeRow));
    v.prefix = c.take(R * P * K * sizeof(int32_t)); v.ret = c.take(R * P * sizeof(double)); v.leaf = c.take(R * P * 2 * sizeof(int32_t));
    v.best = c.take(R * K * sizeof(int32_t)); v.legal = c.take(R * (size_t)b->legal_words * sizeof(uint64_t));
    v.nlegal = c.take(R * sizeof(int32_t)); v.prior = c.take(R * K * sizeof(float));
    v.key = keyed ? c.take(R * sizeof(XrTreeKey)) : 0;
    v.bytes = c.off;
    return v;
}

// xr_batch_tree_open (keep false) and xr_batch_tree_reopen (keep: the session is keyed and may continue from the pool's last one; played,
// kept_out: its two own arguments): one prologue, one carve, one table cache; fn: the entry point, named by every refusal
int32_t eval_open_impl(xr_batch* b, const char* fn, bool keep, int32_t group, const int32_t* played_dev, int32_t n_par, int32_t node_cap, double c_init,
                       double c_base, int32_t max_sims, const float* root_prior_dev, int32_t k_cap, int32_t* kept_out_dev, void* stream) {
    if (!b) return fail(XR_ERR_INVALID, "%s: null argument", fn);
    if (!b->loaded) return fail(XR_ERR_STATE, "%s: load regions first", fn);
    int lo, rows;
    if (const int32_t rc = group_rows(b, group, fn, lo, rows)) return rc;
    if (!std::isfinite(c_init)) return fail(XR_ERR_INVALID, "%s: c_init is not finite", fn);
    if (!tree_knobs_ok(c_init, c_base)) return fail(XR_ERR_INVALID, "%s: c_base must be finite and > 0", fn);
    if (n_par < 1 || n_par > XR_PEEK_MAX) return fail(XR_ERR_RANGE, "%s: n_par %d outside 1..%d", fn, n_par, XR_PEEK_MAX);
    if (max_sims < n_par || max_sims > XR_TREE_MAX_SIMS)
        return fail(XR_ERR_RANGE, "%s: max_sims %d outside n_par %d..%d", fn, max_sims, n_par, XR_TREE_MAX_SIMS);
    if (node_cap < 1) return fail(XR_ERR_RANGE, "%s: node_cap %d < 1", fn, node_cap);
    if (k_cap < b->k_max) return fail(XR_ERR_RANGE, "%s: k_cap %d < k_max %d", fn, k_cap, b->k_max);
    if (const int32_t rc = lds_field_check(b, fn)) return rc;
    const int64_t tasks = (int64_t)rows * n_par;
    if (tasks >= ((int64_t)1 << 31)) return fail(XR_ERR_RANGE, "%s: rows x n_par does not fit 31 bits", fn);
    if (!xr_lookahead_occupancy || !xr_launch_line || !xr_launch_tree_eval_open || !xr_launch_tree_eval_select || !xr_launch_tree_eval_backup ||
        (keep && !xr_launch_tree_eval_reopen))
        return fail(XR_ERR_STATE, "%s: evaluated tree search kernels not linked", fn);
    if (k_cap < 1) k_cap = 1;
    if ((double)rows * ((keep ? 2.0 : 1.0) * (double)node_cap * sizeof(XrTreeNode) + (double)n_par * (4.0 * k_cap + 16.0) + 8.0 * k_cap + 8.0 * b->legal_words +
                        44.0 + (keep ? 24.0 : 0.0) + 160.0) > 1e15)
        return fail(XR_ERR_NOMEM, "%s: %d rows x %d nodes do not fit any device", fn, rows, node_cap);
    const EvalCarve cv = eval_carve(b, rows, n_par, node_cap, k_cap, keep);
    ShadowCall sc;          // (the peek launches of the session play in the caller's shadow slots)
    if (const int32_t rc = shadow_call(b, group, lo, rows, stream, fn, true, sc)) return rc;
    hipStream_t st = sc.st;
    xr_batch::EvalPool& ep = b->eval[group + 1];
    // what a reopen may keep: the trees of a keyed session of this very shape with no wave waiting for its backup (pending visits would
    // be in its nodes); anything else, and a call without `played`, rebuilds every row: the kernel gets played == NULL
    bool rebuild_all = !keep || !played_dev || !ep.keyed || ep.pending || ep.rows != rows || ep.lo != lo || ep.d.n_par != n_par || ep.d.node_cap != node_cap ||
                       ep.d.k_cap != k_cap || ep.d.legal_words != b->legal_words;
    ep.open = false; ep.pending = false; ep.keyed = false;          // the last session ends here, whatever becomes of this call
    if (ep.mem.n < cv.bytes) {
        rebuild_all = true;          // (a new allocation holds no tree)
        if (ep.mem.alloc(cv.bytes) != hipSuccess) {
            ep.mem.release();
            return fail(XR_ERR_NOMEM, "%s: hipMalloc of %zu bytes of trees failed", fn, cv.bytes);
        }
    }
    // a keyed session's table runs to XR_TREE_MAX_SIMS, as the kept search's does: a carried root meets visit counts above max_sims
    const int e_max = keep ? XR_TREE_MAX_SIMS : max_sims;
    const double* E = nullptr;
    if (const int32_t rc = exploration_table(ep.tables, c_init, c_base, e_max, TABLE_EXACTLY, st, fn, E)) return rc;
    uint8_t* const m = ep.mem.p;
    const int old_half = rebuild_all ? 1 : ep.half, new_half = keep ? old_half ^ 1 : 0;          // (nothing refuses from here on)
    XrTreeEvalDev d{};
    d.nodes = reinterpret_cast<XrTreeNode*>(m + cv.half[new_half]); d.rs = reinterpret_cast<XrTreeRow*>(m + cv.rs);
    d.prefix = reinterpret_cast<int32_t*>(m + cv.prefix); d.ret = reinterpret_cast<double*>(m + cv.ret);
    d.leaf = reinterpret_cast<int32_t*>(m + cv.leaf); d.best_order = reinterpret_cast<int32_t*>(m + cv.best);
    d.legal = reinterpret_cast<uint64_t*>(m + cv.legal); d.nlegal = reinterpret_cast<int32_t*>(m + cv.nlegal);
    d.prior = reinterpret_cast<float*>(m + cv.prior);
    d.E = E;
    d.node_cap = node_cap; d.n_par = n_par; d.k_cap = k_cap; d.e_max = e_max; d.env_lo = lo; d.legal_words = b->legal_words;
    d.has_prior = root_prior_dev ? 1 : 0;
    if (keep) {
        XrTreeKeepDev kd{};
        kd.old_nodes = reinterpret_cast<const XrTreeNode*>(m + cv.half[old_half]);
        kd.key = reinterpret_cast<XrTreeKey*>(m + cv.key); kd.key_legal = d.legal;          // the snapshot is the key's legal words
        kd.played = rebuild_all ? nullptr : played_dev; kd.kept_out = kept_out_dev; kd.n_add = max_sims;
        XR_HIP(xr_launch_tree_eval_reopen(&b->dev, &d, &kd, root_prior_dev, rows, st));
        ep.halves[0] = reinterpret_cast<XrTreeNode*>(m + cv.half[0]); ep.halves[1] = reinterpret_cast<XrTreeNode*>(m + cv.half[1]);
        ep.key = kd.key; ep.half = new_half;
    } else {
        XR_HIP(xr_launch_tree_eval_open(&b->dev, &d, root_prior_dev, rows, st));
    }
    ep.keyed = keep;          // (a session started by xr_batch_tree_open is not keyed: the next reopen rebuilds every row)
    ep.d = d; ep.rows = rows; ep.lo = lo; ep.max_sims = max_sims; ep.sims = 0; ep.open = true;
    return XR_OK;
}
}  // namespace

int32_t xr_batch_tree_open(xr_batch* b, int32_t group, int32_t n_par, int32_t node_cap, double c_init, double c_base, int32_t max_sims,
                           const float* root_prior_dev, int32_t k_cap, void* stream) {
    return eval_open_impl(b, "xr_batch_tree_open", false, group, nullptr, n_par, node_cap, c_init, c_base, max_sims, root_prior_dev, k_cap, nullptr, stream);
}

int32_t xr_batch_tree_reopen(xr_batch* b, int32_t group, const int32_t* played_dev, int32_t n_par, int32_t node_cap, double c_init, double c_base,
                             int32_t max_sims, const float* root_prior_dev, int32_t k_cap, int32_t* kept_out_dev, void* stream) {
    return eval_open_impl(b, "xr_batch_tree_reopen", true, group, played_dev, n_par, node_cap, c_init, c_base, max_sims, root_prior_dev, k_cap, kept_out_dev, stream);
}

int32_t xr_batch_tree_leaves(xr_batch* b, int32_t group, uint8_t* rows_out_dev, int64_t row_bytes, int32_t region_base, int32_t* out_dev,
                             double* return_out_dev, int32_t* paths_out_dev, int32_t* leaf_out_dev, void* stream) {
    const char* fn = "xr_batch_tree_leaves";
    if (!b || !rows_out_dev || !out_dev) return fail(XR_ERR_INVALID, "%s: null argument", fn);
    if (const int32_t rc = state_row_check(b, fn, rows_out_dev, row_bytes, ROWS_ALIGNED)) return rc;
    if (!b->loaded) return fail(XR_ERR_STATE, "%s: load regions first", fn);
    int lo, rows;
    if (const int32_t rc = group_rows(b, group, fn, lo, rows)) return rc;
    if (const int32_t rc = state_row_check(b, fn, rows_out_dev, row_bytes, ROWS_LONG)) return rc;
    if (const int32_t rc = lds_field_check(b, fn)) return rc;
    xr_batch::EvalPool& ep = b->eval[group + 1];
    if (!ep.open || ep.rows != rows || ep.lo != lo || ep.d.legal_words != b->legal_words)
        return fail(XR_ERR_STATE, "%s: no open session of this caller (xr_batch_tree_open first)", fn);
    if (ep.pending) return fail(XR_ERR_STATE, "%s: the last wave's leaves still wait for xr_batch_tree_backup", fn);
    if (ep.sims + ep.d.n_par > ep.max_sims)
        return fail(XR_ERR_RANGE, "%s: %d simulations so far, a wave of %d would pass max_sims %d", fn, ep.sims, ep.d.n_par, ep.max_sims);
    if (!xr_lookahead_occupancy || !xr_launch_line || !xr_launch_tree_eval_select) return fail(XR_ERR_STATE, "%s: evaluated tree search kernels not linked", fn);
    ShadowCall c;
    if (const int32_t rc = shadow_call(b, group, lo, rows, stream, fn, true, c)) return rc;
    hipStream_t st = c.st;
    const int64_t tasks = (int64_t)rows * ep.d.n_par;
    XR_HIP(xr_launch_tree_eval_select(&ep.d, paths_out_dev, leaf_out_dev, rows, st));
    ep.pending = true;          // (the paths carry pending visits from here on: only a backup, or a new open, clears them)
    XrLineLaunch l{};           // the wave's paths as prefixes, no policy after them: the rows of the leaves, their line returns into the pool
    l.kind = XR_LINE_PEEK; l.per_row = ep.d.n_par;
    l.prefix = ep.d.prefix; l.prefix_stride = ep.d.k_cap;
    l.rows = rows_out_dev; l.row_bytes = row_bytes; l.region_base = region_base;
    l.out = out_dev; l.return_out = ep.d.ret;
    XR_HIP(launch_line(b, c, l));
    if (return_out_dev) XR_HIP(hipMemcpyAsync(return_out_dev, ep.d.ret, (size_t)tasks * sizeof(double), hipMemcpyDeviceToDevice, st));
    return XR_OK;
}

int32_t xr_batch_tree_backup(xr_batch* b, int32_t group, const double* value_dev, const float* leaf_prior_dev, int32_t* visits_out_dev,
                             double* value_out_dev, int32_t* info_out_dev, int32_t* best_order_out_dev, double* best_return_out_dev,
                             double* returns_out_dev, void* stream) {
    const char* fn = "xr_batch_tree_backup";
    if (!b || !value_dev || !visits_out_dev || !value_out_dev || !info_out_dev) return fail(XR_ERR_INVALID, "%s: null argument", fn);
    if (!b->loaded) return fail(XR_ERR_STATE, "%s: load regions first", fn);
    int lo, rows;
    if (const int32_t rc = group_rows(b, group, fn, lo, rows)) return rc;
    xr_batch::EvalPool& ep = b->eval[group + 1];
    if (!ep.open || !ep.pending || ep.rows != rows || ep.lo != lo)
        return fail(XR_ERR_STATE, "%s: no pending leaves of this caller (xr_batch_tree_leaves first)", fn);
    if (!xr_launch_tree_eval_backup) return fail(XR_ERR_STATE, "%s: evaluated tree search kernels not linked", fn);
    XR_HIP(hipSetDevice(b->cfg.device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    XR_HIP(xr_launch_tree_eval_backup(&ep.d, value_dev, leaf_prior_dev, ep.sims + ep.d.n_par, visits_out_dev, value_out_dev, info_out_dev, best_order_out_dev,
                                      best_return_out_dev, returns_out_dev, rows, st));
    ep.sims += ep.d.n_par;
    ep.pending = false;
    return XR_OK;
}

// ---- branch ------------------------------------------------------------------------------------------------------------------------
int32_t xr_batch_branch(xr_batch* b, int32_t group, const int32_t* parent_dev, void* stream) {
    if (!b || !parent_dev) return fail(XR_ERR_INVALID, "xr_batch_branch: null argument");
    if (!b->loaded) return fail(XR_ERR_STATE, "xr_batch_branch: load regions first");
    int lo, rows;
    if (const int32_t rc = group_rows(b, group, "xr_batch_branch", lo, rows)) return rc;
    if (!xr_launch_branch) return fail(XR_ERR_STATE, "xr_batch_branch: branch kernels not linked");
    XR_HIP(hipSetDevice(b->cfg.device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    xr_batch::BranchPool& bp = b->branch[group + 1];
    if (bp.rows < rows) {              // the first branch of this caller (or its group has grown since: xr_batch_set_groups)
        bp.release();
        Carver size, place;            // the staging rows: one slot of every state row per row of the caller
        carve_slots(b, size, nullptr, bp.stg, (size_t)rows);
        if (bp.mem.alloc(size.off) != hipSuccess) {
            bp.release();
            return fail(XR_ERR_NOMEM, "xr_batch_branch: hipMalloc of %zu bytes of staging rows failed", size.off);
        }
        bp.rows = rows;
        carve_slots(b, place, bp.mem.p, bp.stg, (size_t)rows);
    }
    // workgroups per row: about 4 KB of the two long rows each (one 16-byte vector per thread), fewer once the rows alone fill the chip
    const size_t long_bytes = (size_t)b->n_max * sizeof(int16_t) + (size_t)b->path_cap * sizeof(int32_t);
    int chunks = (int)std::min<size_t>(32, std::max<size_t>(1, long_bytes / 4096));
    if ((int64_t)rows * chunks > 16384) chunks = std::max(1, 16384 / rows);
    // the state of slots changes: no caller buffer holds their observation any more (a group call: the group's and the batch-wide one)
    if (group < 0) {
        drop_obs_valid(b);
    } else {
        b->obs_valid.clear();
        b->group_valid[group].clear();
    }
    XrSlotRows env{};
    copy_slot_rows(env, b->dev);
    XR_HIP(xr_launch_branch(&env, &bp.stg, lo, rows, parent_dev, b->n_max, b->path_cap, b->legal_words, chunks, st));
    return XR_OK;
}

int32_t xr_observation_from_records(const uint32_t* nodes_dev, int32_t X, int32_t Y, int32_t Z, const int32_t* nets_dev,
                                    int32_t k, float* out_dev, void* stream) {
    if (!nodes_dev || !out_dev || (k > 0 && !nets_dev)) return fail(XR_ERR_INVALID, "xr_observation_from_records: null argument");
    if (X < 1 || Y < 1 || Z < 1 || (int64_t)X * Y * Z > ((int64_t)1 << 30) || k < 0 || k > 15000)
        return fail(XR_ERR_RANGE, "xr_observation_from_records: dims %dx%dx%d / k %d out of range", X, Y, Z, k);
    const int N = X * Y * Z;
    const bool vec4 = (N % 4 == 0) && ((reinterpret_cast<uintptr_t>(out_dev) & 15) == 0);
    XR_HIP(xr_launch_obs_records(nodes_dev, X, Y, Z, nets_dev, k, out_dev, vec4 ? 1 : 0, static_cast<hipStream_t>(stream)));
    return XR_OK;
}

}  // extern "C"
