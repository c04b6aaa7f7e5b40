// tests/hostsan/load_trace.cpp — TEST INFRASTRUCTURE (see hip/hip_runtime.h of this directory).
//
// Prints, as text, everything xr_batch_load_regions decides and uploads, for a list of cases that takes every branch of the loader: the
// return code and message, xr_batch_sizes, xr_batch_route_occupancy, the size of every hipMalloc in order, and — at the first route launch
// after the load — the router variant, XrBatchDev field by field, the region table, and a hash of every static table.  "Device" memory is
// host memory here, so the launch hook of stub_launch.cpp can read all of it back.  tests/test_load_trace.py compares the output with
// load_trace.expected, recorded before the loader was split into steps: any change of what the loader decides shows as a diff of named
// fields.  Drives the public C ABI only; runs under ASan + UBSan as a program of its own (no preload).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/xroute_hip.h"
#include "../../xroute_env_amd/csrc/xr_device.h"

extern "C" void (*xr_stub_launch_hook)(const char* name, const XrBatchDev* b, const XrRouteVariant* v);

namespace {

struct Lcg {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)(s >> 33); }
    int below(int n) { return (int)(next() % (uint32_t)n); }
};

struct Reg {
    int X = 0, Y = 0, Z = 0, K = 0;
    std::vector<int32_t> xs, ys;
    std::vector<uint8_t> dir;
    std::vector<uint32_t> nodes;
    int64_t N() const { return (int64_t)X * Y * Z; }
    xr_region_desc desc() const {
        xr_region_desc d{};
        d.dim_x = X; d.dim_y = Y; d.dim_z = Z;
        d.xs_host = xs.data(); d.ys_host = ys.data(); d.layer_dir_host = dir.data(); d.nodes_host = nodes.data();
        d.n_nets = K;
        d.metrics0[0] = K; d.metrics0[1] = 10 * X; d.metrics0[2] = Y;
        return d;
    }
};

uint32_t rec(uint32_t type, int net1, int pin1) { return type | ((uint32_t)net1 << 3) | ((uint32_t)pin1 << 17); }

// Blockages on blk_pm per mille of the nodes; every net but each fifth (those keep no access point) gets 2-4 pins of 1-2 access points
// near a centre; one pin in four is walled in by blockages (the closed pockets of the per-net facts)
Reg gen(uint64_t seed, int X, int Y, int Z, int K, int xstep = 400, int ystep = 380, int blk_pm = 30) {
    Lcg g{seed * 2654435761ULL + 12345};
    Reg r;
    r.X = X; r.Y = Y; r.Z = Z; r.K = K;
    for (int i = 0; i < X; i++) r.xs.push_back(i ? r.xs.back() + xstep + 20 * g.below(3) : 1000 + g.below(100));
    for (int i = 0; i < Y; i++) r.ys.push_back(i ? r.ys.back() + ystep + 10 * g.below(4) : -500 + g.below(100));
    for (int z = 0; z < Z; z++) r.dir.push_back((uint8_t)((z + (int)(seed & 1)) & 1));
    const int N = (int)r.N(), YZ = Y * Z;
    r.nodes.assign(N, XR_TYPE_NORMAL);
    for (int i = 0; i < (int)((int64_t)N * blk_pm / 1000); i++) r.nodes[g.below(N)] = XR_TYPE_BLOCKAGE;
    for (int n = 1; n <= K; n++) {
        if (n % 5 == 0) continue;
        const int pins = 2 + g.below(3), cx = g.below(X), cy = g.below(Y);
        for (int p = 1; p <= pins; p++) {
            const bool wall = g.below(4) == 0;
            for (int a = 1 + g.below(2); a > 0; a--) {
                const int x = std::min(X - 1, std::max(0, cx + g.below(5) - 2)), y = std::min(Y - 1, std::max(0, cy + g.below(5) - 2)), z = g.below(Z);
                const int f = (x * Y + y) * Z + z;
                if (r.nodes[f] != XR_TYPE_NORMAL) continue;
                r.nodes[f] = rec(XR_TYPE_ACCESS, n, p);
                if (!wall) continue;
                const int nb[6] = {x + 1 < X ? f + YZ : -1, x > 0 ? f - YZ : -1, y + 1 < Y ? f + Z : -1, y > 0 ? f - Z : -1, z + 1 < Z ? f + 1 : -1, z > 0 ? f - 1 : -1};
                for (int q : nb)
                    if (q >= 0 && r.nodes[q] == XR_TYPE_NORMAL) r.nodes[q] = XR_TYPE_BLOCKAGE;
            }
        }
    }
    return r;
}

uint64_t fnv(const void* p, size_t bytes) {
    uint64_t h = 0xcbf29ce484222325ULL;
    const uint8_t* q = static_cast<const uint8_t*>(p);
    for (size_t i = 0; i < bytes; i++) h = (h ^ q[i]) * 0x100000001b3ULL;
    return h;
}

// ---- what the hooks see -------------------------------------------------------------------------------------------------------------
enum { kOff, kStep, kObserve };
int g_mode = kOff;
bool g_full = false;
std::vector<size_t> g_mallocs;
struct Seen { bool step = false, observe = false; int kzch = 0, lds = 0, win = 0, obs_zch = 0, obs_vec4 = 0; } g_seen;

void on_malloc(size_t bytes) { g_mallocs.push_back(bytes); }

void print_mallocs(const char* when) {
    printf("  hipMalloc %s (%zu):", when, g_mallocs.size());
    for (size_t n : g_mallocs) printf(" %zu", n);
    printf("\n");
    g_mallocs.clear();
}

void print_variant(const char* name, const XrRouteVariant* v) {
    printf("  %s variant: lds_dist=%d zch=%d lds_bytes=%zu threads=%d\n", name, v->lds_dist, v->zch, v->lds_bytes, v->threads);
}

void dump_dev(const XrBatchDev* d) {
    int col = 0;
    auto sep = [&] { if (++col % 8 == 0) printf("\n   "); };
#define S(f) printf(" " #f "=%lld", (long long)d->f), sep()
#define U(f) printf(" " #f "=%llu", (unsigned long long)d->f), sep()
#define F(f) printf(" " #f "=%.17g", d->f), sep()
    printf("  dev:");
    S(meas_shift); S(heavy_class); S(heavy_mult); S(n_regions); S(n_envs); S(n_max); S(n_lds); S(lw_max); S(lines_max); S(x_max); S(y_max);
    S(legal_words); S(path_cap); S(obs_stride); S(obs_vec4); S(obs_head_only); S(obs_incremental); S(obs_split_pm); S(queue_quota_pm);
    S(queue_skip_shift); S(obs_lds_bytes); S(queue_grid); S(via_cost); S(pen_cost); S(max_route_count); S(auto_reset); S(env_base); S(env_count);
    S(guide_cost); S(guide_margin); S(maze_end_iter); S(dial_mult_big); S(dial_mult); S(round_cap); S(win_x); S(win_y); S(win_nmax); S(win_margin);
    S(win_ystep); U(win_m24_yz); U(win_m24_z); U(win_m24_mw); U(win_s24); F(w_violation); F(w_via); F(w_wirelength);
    printf("\n  null:");
#define P(f) if (!d->f) printf(" " #f)
    P(regions); P(rg_rec); P(rg_node_net); P(rg_owner0); P(coords); P(net_csr); P(ap_node); P(ap_pin); P(ap_feat); P(legal0); P(net_work); P(net_meas);
    P(net_info); P(ap_flags); P(guide_csr); P(guide_box); P(guide_mask); P(env_region); P(env_replay); P(owner); P(legal); P(nlegal); P(cum); P(delta);
    P(reward); P(done); P(status); P(path); P(path_len); P(hash); P(env_steps); P(total_steps); P(sweeps); P(touched); P(records); P(dist_scratch);
    P(cls_scratch); P(list_scratch); P(dg_field); P(dg_masks); P(dg_touch); P(dg_path); P(phase_cycles); P(obs_out); P(plan_region); P(plan_units);
    P(plan_unit_net); P(queue); P(route_order); P(obs_out_u8);
    printf("\n");
#undef S
#undef U
#undef F
#undef P
    for (int r = 0; r < d->n_regions; r++) {
        const XrRegionDev& R = d->regions[r];
        printf("  region %d: X=%d Y=%d Z=%d N=%d n_nets=%d nlegal0=%d m0=%d,%d,%d ldir_mask=%u xs_off=%d ys_off=%d net_off=%d ap_off=%d node_off=%lld legal0_off=%lld\n"
               "    w_min=%u magic_yz=%u magic_z=%u magic_mw=%u m24_yz=%u m24_z=%u m24_mw=%u s24=%u gmask_off=%lld gmask_stride=%d pad0=%d\n",
               r, R.X, R.Y, R.Z, R.N, R.n_nets, R.nlegal0, R.m0[0], R.m0[1], R.m0[2], R.ldir_mask, R.xs_off, R.ys_off, R.net_off, R.ap_off, (long long)R.node_off,
               (long long)R.legal0_off, R.w_min, R.magic_yz, R.magic_z, R.magic_mw, R.m24_yz, R.m24_z, R.m24_mw, R.s24, (long long)R.gmask_off, R.gmask_stride, R.pad0);
    }
    // lengths from the region table: the last region ends every table
    const XrRegionDev& L = d->regions[d->n_regions - 1];
    const size_t n_coords = (size_t)L.ys_off + L.Y, n_csr = (size_t)L.net_off + L.n_nets + 2, n_ap = (size_t)L.ap_off + d->net_csr[n_csr - 1];
    const size_t n_rec = ((size_t)L.node_off + L.N + 7) & ~(size_t)7, B = (size_t)d->n_envs, mwg = (size_t)d->n_max / 32 + 1;
    printf("  lengths: coords=%zu csr=%zu ap=%zu rec=%zu\n", n_coords, n_csr, n_ap, n_rec);
#define H(f, bytes) printf(" " #f "=%016llx", (unsigned long long)fnv(d->f, (bytes)))
    printf("  hash:");
    H(coords, n_coords * 4); H(net_csr, n_csr * 4); H(ap_node, n_ap * 4); H(ap_pin, n_ap * 2); H(ap_feat, n_ap * 4); H(ap_flags, n_ap); H(net_info, n_csr * 4);
    printf("\n   ");
    H(net_work, n_csr); H(legal0, (size_t)d->n_regions * d->legal_words * 8); H(rg_rec, n_rec * 4); H(env_region, B * 4); H(hash, B * 8);
    if (d->dg_field) { H(dg_field, B * d->n_max * 4); H(dg_masks, B * 2 * mwg * 4); }
    printf("\n");
#undef H
}

void on_launch(const char* name, const XrBatchDev* b, const XrRouteVariant* v) {
    if (g_mode == kOff) return;
    printf("  launch %s\n", name);
    if (!v || !b) return;
    if (g_mode == kStep && !strcmp(name, "route")) {
        print_variant("step", v);
        g_seen.step = true; g_seen.kzch = v->zch; g_seen.lds = v->lds_dist; g_seen.win = b->win_x;
        if (g_full) dump_dev(b);
    } else if (g_mode == kObserve) {
        print_variant("observe", v);
        printf("  observe dev: obs_vec4=%d obs_head_only=%d obs_incremental=%d obs_lds_bytes=%d queue_grid=%d route_order=%s\n", b->obs_vec4, b->obs_head_only,
               b->obs_incremental, b->obs_lds_bytes, b->queue_grid, b->route_order ? "set" : "null");
        g_seen.observe = true; g_seen.obs_zch = v->zch; g_seen.obs_vec4 = b->obs_vec4;
    }
    g_mode = kOff;
}

// ---- one load, traced ---------------------------------------------------------------------------------------------------------------
std::map<std::string, int> g_reached;       // what the cases reached (the coverage the program asserts at its end)
int g_failures = 0;

void check(bool ok, const char* what) {
    if (ok) return;
    printf("  TRACE FAILURE: %s\n", what);
    g_failures++;
}

// returns the load's return code; g_seen holds what the launches showed
int32_t load_traced(xr_batch* h, const std::vector<const Reg*>& regs, bool full, bool guides = true) {
    std::vector<xr_region_desc> descs;
    bool mult4 = true;
    for (const Reg* r : regs) { descs.push_back(r->desc()); mult4 = mult4 && r->N() % 4 == 0; }
    g_seen = Seen{};
    g_full = full;
    g_mallocs.clear();
    const int32_t rc = xr_batch_load_regions(h, descs.data(), (int32_t)descs.size(), nullptr);
    printf("  load rc=%d error=\"%s\"\n", rc, rc ? xr_last_error() : "");
    print_mallocs("load");
    int32_t s[6] = {0, 0, 0, 0, 0, 0}, per_cu = 0;
    int64_t stride = 0, lds = 0;
    const int32_t rs = xr_batch_sizes(h, &s[0], &s[1], &s[2], &s[3], &s[4], &s[5], &stride);
    printf("  sizes rc=%d n_envs=%d n_regions=%d n_max=%d k_max=%d legal_words=%d path_cap=%d obs_env_stride=%lld\n", rs, s[0], s[1], s[2], s[3], s[4], s[5], (long long)stride);
    const int32_t ro = xr_batch_route_occupancy(h, &per_cu, &lds);
    printf("  occupancy rc=%d workgroups_per_cu=%d lds_bytes=%lld\n", ro, per_cu, (long long)lds);
    check((rc == XR_OK) == (rs == XR_OK) && rs == ro, "sizes / occupancy answer like the load");
    if (rc != XR_OK) return rc;
    std::vector<int32_t> actions(s[0], 1);
    alignas(16) static float out[4];
    g_mode = kStep;
    const int32_t r1 = xr_batch_step(h, actions.data(), nullptr);
    g_mode = kObserve;
    const int32_t r2 = xr_batch_step_observe(h, actions.data(), out, stride, nullptr);
    g_mode = kOff;
    printf("  step rc=%d step_observe rc=%d\n", r1, r2);
    check(r1 == XR_OK && r2 == XR_OK && g_seen.step && g_seen.observe, "a route launch and an observe launch were seen");
    print_mallocs("steps");
    if (g_seen.kzch < 0 && g_seen.obs_zch >= 0) g_reached["sweep_full"]++;
    if (!mult4 && g_seen.obs_vec4 == 0) g_reached["stream_ok=false"]++;       // (aligned rows, some N % 4 != 0: the shifted float4 form needs stream_ok)
    if (g_seen.win > 0) g_reached["window"]++;
    if (guides && regs[0]->K >= 1) {       // one box, net 1 of region 0
        std::vector<int32_t> off(regs[0]->K + 1, 1);
        off[0] = 0;
        const int16_t box[6] = {0, 0, (int16_t)(regs[0]->X - 1), (int16_t)(regs[0]->Y - 1), 0, (int16_t)(regs[0]->Z - 1)};
        std::vector<const int32_t*> offs(regs.size(), nullptr);
        std::vector<const int16_t*> boxes(regs.size(), nullptr);
        offs[0] = off.data(); boxes[0] = box;
        const int32_t rg = xr_batch_load_guides(h, offs.data(), boxes.data(), nullptr);
        printf("  load_guides rc=%d error=\"%s\"\n", rg, rg ? xr_last_error() : "");
        print_mallocs("guides");
    }
    return rc;
}

std::string kzch_key(int kzch, int lds) {
    std::string k = "kzch=" + std::to_string(kzch);
    if (kzch == -1) k += lds ? " (LDS)" : " (scratch)";      // the bucketed-frontier router has both forms
    return k;
}

xr_config config(int n_envs = 2) {
    xr_config c;
    xr_config_default(&c);
    c.n_envs = n_envs;
    return c;
}

// A case on a batch of its own.  `reaches`: the mark of the case — the router form it must take ("kzch=..."), or "rc=<code>" for a refusal
void run_case(const char* name, const xr_config& cfg, const std::vector<const Reg*>& regs, const std::string& reaches, bool full = true) {
    printf("case %s [%s]\n", name, reaches.c_str());
    xr_batch* h = nullptr;
    const int32_t rc0 = xr_batch_create(&cfg, &h);
    if (rc0 != XR_OK) { printf("  create rc=%d error=\"%s\"\n", rc0, xr_last_error()); check(false, "create"); return; }
    const int32_t rc = load_traced(h, regs, full);
    const std::string got = rc == XR_OK ? kzch_key(g_seen.kzch, g_seen.lds) : "rc=" + std::to_string(rc);
    if (got != reaches) printf("  reached %s\n", got.c_str());
    check(got == reaches, "the case reaches what it is marked with");
    g_reached[got]++;
    xr_batch_destroy(h);
    check(xr_stub_alloc_live == 0, "no device buffer outlives the batch");
}

// ---- the numeric thresholds of the router choice (place_route, choose_window) and of check_desc, each from both sides ------------------
// Tracks from their gaps: the case decides every coordinate
void retrack(std::vector<int32_t>& t, const std::vector<int64_t>& gaps, int64_t origin) {
    t.assign(1, (int32_t)origin);
    int64_t c = origin;
    for (int64_t g : gaps) t.push_back((int32_t)(c += g));
}
Reg with_x(Reg r, const std::vector<int64_t>& gaps, int64_t origin = 0) { retrack(r.xs, gaps, origin); return r; }
Reg with_y(Reg r, const std::vector<int64_t>& gaps, int64_t origin = 0) { retrack(r.ys, gaps, origin); return r; }
// n - 1 gaps of `pitch`, the one in the middle `wide`
std::vector<int64_t> one_wide(int n, int64_t wide, int64_t pitch = 400) {
    std::vector<int64_t> g(n - 1, pitch);
    g[(n - 1) / 2] = wide;
    return g;
}
// n - 1 nearly equal gaps that span `ext`
std::vector<int64_t> spanning(int n, int64_t ext) {
    std::vector<int64_t> g(n - 1, ext / (n - 1));
    g.back() = ext - (ext / (n - 1)) * (n - 2);
    return g;
}

void range_case(const char* name, const xr_config& cfg, const std::vector<const Reg*>& regs, const std::string& reaches, int win_x = 0) {
    run_case(name, cfg, regs, reaches, false);
    if (reaches.compare(0, 3, "rc=") == 0) return;
    printf("  seen: zch=%d lds_dist=%d win_x=%d\n", g_seen.kzch, g_seen.lds, g_seen.win);
    check(g_seen.win == win_x, "the window the case is marked with");
}

void range_cases() {
    g_reached.clear();
    const Reg a662 = gen(1, 6, 6, 2, 3), r4040 = gen(12, 40, 40, 9, 5), r6448 = gen(7, 64, 48, 12, 6);
    const int64_t step = XR3_STEP_LIMIT, extent = XR3_EXTENT_LIMIT, pen = 3200;       // (the default penalty: drc_cost 8 x drc_unit 400)
    const std::vector<int64_t> p400(5, 400);
    xr_config c, v2 = config();
    v2.maze_end_iter = 2;                                                             // pen_max = 6400
    Reg r, q;
    // edge_max + pen_max + guide_cost against 2^20: the largest term a pitch in x, a pitch in y, the via, the penalty, the guide cost
    r = with_x(a662, one_wide(6, step - 1 - pen));
    range_case("step 2^20 - 1, a pitch in x", config(), {&r}, "kzch=-3");
    r = with_x(a662, one_wide(6, step - pen));
    range_case("step 2^20, a pitch in x", config(), {&r}, "kzch=-1 (LDS)");
    r = with_y(a662, one_wide(6, step - 1 - pen));
    range_case("step 2^20 - 1, a pitch in y", config(), {&r, &a662}, "kzch=-3");
    r = with_y(a662, one_wide(6, step - pen));
    range_case("step 2^20, a pitch in y", config(), {&a662, &r}, "kzch=-1 (LDS)");
    r = with_x(a662, one_wide(6, step - 1 - 2 * pen));
    range_case("step 2^20 - 1, a pitch in x, maze_end_iter 2", v2, {&r}, "kzch=-4");
    r = with_x(a662, one_wide(6, step - 2 * pen));
    range_case("step 2^20, a pitch in x, maze_end_iter 2", v2, {&r}, "kzch=-2");
    c = config(); c.via_cost = (int32_t)(step - 1 - pen);
    range_case("step 2^20 - 1, the via", c, {&a662}, "kzch=-3");
    c.via_cost = (int32_t)(step - pen);
    range_case("step 2^20, the via", c, {&a662}, "kzch=-1 (LDS)");
    c = config(); c.drc_unit = 1; c.drc_cost = (int32_t)(step - 1 - 800);              // (edge_max: the via, 800)
    range_case("step 2^20 - 1, the penalty", c, {&a662}, "kzch=-3");
    c.drc_cost = (int32_t)(step - 800);
    range_case("step 2^20, the penalty", c, {&a662}, "kzch=-1 (LDS)");
    c = config(); c.drc_unit = 1; c.drc_cost = (int32_t)((step - 4 - 800) >> 2); c.maze_end_iter = 3;
    range_case("step 2^20 - 4, the penalty of attempt 3", c, {&a662}, "kzch=-4");
    c.drc_cost = (int32_t)((step - 800) >> 2);
    range_case("step 2^20, the penalty of attempt 3", c, {&a662}, "kzch=-2");
    c = config(); c.guide_cost = (int32_t)(step - 1 - pen - 800);
    range_case("step 2^20 - 1, the guide cost", c, {&a662}, "kzch=-4");
    c.guide_cost = (int32_t)(step - pen - 800);
    range_case("step 2^20, the guide cost", c, {&a662}, "kzch=-2");
    // ext_max against 2^25, every single edge far below 2^20
    r = with_x(r4040, spanning(40, extent - 1));
    range_case("extent 2^25 - 1 in x", config(), {&r}, "kzch=-3");
    range_case("extent 2^25 - 1 in x, maze_end_iter 2", v2, {&r}, "kzch=-4");
    r = with_x(r4040, spanning(40, extent));
    range_case("extent 2^25 in x", config(), {&r}, "kzch=-1 (LDS)");
    range_case("extent 2^25 in x, maze_end_iter 2", v2, {&r}, "kzch=-2");
    r = with_y(r4040, spanning(40, extent - 1), -(1 << 30));
    range_case("extent 2^25 - 1 in y, from -2^30", config(), {&a662, &r}, "kzch=-3");
    r = with_y(r4040, spanning(40, extent), (1 << 30) - extent);
    range_case("extent 2^25 in y, up to 2^30", config(), {&r, &a662}, "kzch=-1 (LDS)");
    // via_cost * 32 against 2^25 (no penalty: the via is an edge, the step limit would decide first)
    c = config(); c.drc_cost = 0; c.via_cost = (int32_t)(step - 1);
    range_case("via_cost 2^20 - 1", c, {&a662}, "kzch=-3");
    c.maze_end_iter = 2;
    range_case("via_cost 2^20 - 1, maze_end_iter 2", c, {&a662}, "kzch=-4");
    c.via_cost = (int32_t)step;
    range_case("via_cost 2^20, maze_end_iter 2", c, {&a662}, "kzch=-2");
    c.maze_end_iter = 1;
    range_case("via_cost 2^20", c, {&a662}, "kzch=-1 (LDS)");
    // the window form's two conditions: edge_max + penalty below 2^20, window tracks x edge_max below 2^25
    c = config(4); c.window = 52;
    r = with_x(r6448, one_wide(64, step - 1 - pen));
    range_case("window 52, step 2^20 - 1: 32 tracks x edge_max stay below 2^25", c, {&r}, "kzch=-1 (scratch)", 32);
    r = with_x(r6448, one_wide(64, step - pen));
    range_case("window 52, step 2^20 (off)", c, {&r}, "kzch=-1 (scratch)", 0);
    r = with_y(r6448, one_wide(48, (extent - 1) / 48));                               // (48 rows: the window has at most 48 tracks)
    range_case("window 52, 48 x edge_max = 2^25 - 32", c, {&r}, "kzch=-1 (scratch)", 48);
    r = with_y(r6448, one_wide(48, (extent - 1) / 48 + 1));
    range_case("window 52, 48 x edge_max = 2^25 + 16: 46 tracks", c, {&r}, "kzch=-1 (scratch)", 46);
    // coordinates in [-2^30, 2^30], both ends included; the span of an axis below 2^28
    r = with_x(a662, p400, -(1 << 30));
    q = with_y(a662, p400, (1 << 30) - 2000);
    range_case("xs from -2^30, ys up to 2^30", config(), {&r, &q}, "kzch=-3");
    r = with_x(a662, one_wide(6, XR_MAX_TRACK_SPAN - 1 - 1600), -(1 << 27));
    range_case("xs span 2^28 - 1", config(), {&r}, "kzch=-1 (LDS)");
    r = with_x(a662, one_wide(6, XR_MAX_TRACK_SPAN - 1600), -(1 << 27));
    range_case("xs span 2^28", config(), {&r}, "rc=-5");
    r = with_y(a662, one_wide(6, XR_MAX_TRACK_SPAN - 1 - 1600));
    c = config(); c.force_scratch_field = 1;
    range_case("ys span 2^28 - 1, force_scratch_field", c, {&a662, &r}, "kzch=-1 (scratch)");
    r = with_y(a662, one_wide(6, XR_MAX_TRACK_SPAN - 1600));
    range_case("ys span 2^28", config(), {&a662, &r}, "rc=-5");
    r = with_x(a662, one_wide(6, ((int64_t)1 << 31) - 1600), -(1 << 30));
    range_case("xs from -2^30 to 2^30 (a span of 2^31)", config(), {&r}, "rc=-5");
    c = config(); c.router = XR_ROUTER_SWEEP;
    r = with_x(a662, one_wide(6, XR_MAX_TRACK_SPAN - 1 - 1600));
    range_case("xs span 2^28 - 1, sweeps", c, {&r}, "kzch=0");

    printf("reached (thresholds):\n");
    for (const auto& kv : g_reached) printf("  %-20s %d\n", kv.first.c_str(), kv.second);
}

}  // namespace

int main() {
    xr_stub_launch_hook = on_launch;
    xr_stub_malloc_hook = on_malloc;
    const Reg a662 = gen(1, 6, 6, 2, 3), b662 = gen(2, 6, 6, 2, 4), r753 = gen(3, 7, 5, 3, 2), r2440 = gen(4, 24, 40, 9, 6), r2440b = gen(5, 24, 40, 9, 5);
    const Reg r2020 = gen(6, 20, 20, 12, 5), r6448 = gen(7, 64, 48, 12, 6), big = gen(8, 64, 64, 16, 4, 400, 380, 2), big2 = gen(9, 64, 72, 16, 3, 400, 380, 2);
    const Reg nets211 = gen(10, 40, 40, 4, 211), wide = gen(11, 6, 6, 2, 3, 1 << 20, 1 << 20), r4040 = gen(12, 40, 40, 9, 5);
    const std::vector<const Reg*> small{&a662, &b662}, mixed{&r2440, &r753, &r2020, &a662};
    xr_config c;

    // ---- the router forms -----------------------------------------------------------------------------------------------------------
    run_case("6x6x2 pair", config(), small, "kzch=-3");
    run_case("7x5x3 (odd N)", config(), {&r753}, "kzch=-3");
    run_case("24x40x9, 64 envs", config(64), {&r2440, &r2440b}, "kzch=-3");
    run_case("20x20x12", config(), {&r2020}, "kzch=-3");
    run_case("mixed layers, 64 envs", config(64), mixed, "kzch=-3");
    run_case("211 nets", config(), {&nets211}, "kzch=-3");
    c = config(); c.router = XR_ROUTER_SWEEP;
    run_case("sweep 24x40x9", c, {&r2440, &r2440b}, "kzch=9");
    run_case("sweep 20x20x12", c, {&r2020}, "kzch=12");
    run_case("sweep mixed layers", c, mixed, "kzch=0");
    c.force_scratch_field = 1;
    run_case("sweep 24x40x9, force_scratch_field", c, {&r2440}, "kzch=9");
    c.block_threads = 128;
    run_case("sweep mixed, force_scratch_field, block_threads 128", c, mixed, "kzch=0", false);
    c = config(); c.router = XR_ROUTER_DIAL;
    run_case("router DIAL 6x6x2 pair", c, small, "kzch=-3", false);
    run_case("router DIAL 64x48x12", c, {&r6448}, "kzch=-1 (scratch)", false);
    c.router = XR_ROUTER_DIAL_R2;
    run_case("router DIAL_R2 24x40x9", c, {&r2440}, "kzch=-1 (LDS)");
    run_case("track pitches of 2^20 (the LDS form's step limit)", config(), {&wide, &a662}, "kzch=-1 (LDS)");
    c = config(); c.force_scratch_field = 1;
    run_case("force_scratch_field 6x6x2 pair", c, small, "kzch=-1 (scratch)");
    c.n_envs = 4096;
    run_case("force_scratch_field, 4096 envs (512 threads)", c, small, "kzch=-1 (scratch)", false);
    run_case("64x48x12", config(4), {&r6448}, "kzch=-1 (scratch)");
    run_case("64x48x12 + 7x5x3 (no stream form)", config(4), {&r6448, &r753}, "kzch=-1 (scratch)");
    run_case("65536 and 73728 nodes (no 24-bit magics)", config(), {&big, &big2}, "kzch=-1 (scratch)");
    run_case("65536 nodes + 6x6x2 (no 24-bit magics)", config(), {&a662, &big}, "kzch=-1 (scratch)", false);
    // ---- XR-Maze v2 -----------------------------------------------------------------------------------------------------------------
    c = config(); c.guide_cost = 200; c.guide_margin = 1;
    run_case("guide_cost 6x6x2 pair", c, small, "kzch=-4");
    run_case("guide_cost 64x48x12", c, {&r6448}, "kzch=-2");
    c = config(); c.maze_end_iter = 3;
    run_case("maze_end_iter 3 mixed", c, mixed, "kzch=-4");
    c.router = XR_ROUTER_DIAL_R2;
    run_case("maze_end_iter 3, DIAL_R2", c, small, "kzch=-2");
    c.router = XR_ROUTER_SWEEP;
    run_case("maze_end_iter 3 without the frontier router", c, small, "rc=-5");
    c = config(); c.guide_cost = 200; c.router = XR_ROUTER_SWEEP;
    run_case("guide_cost without the frontier router", c, small, "rc=-5");
    // ---- window form, workgroup size, knobs -----------------------------------------------------------------------------------------
    c = config(4); c.window = 52;
    run_case("window 52, 64x48x12", c, {&r6448}, "kzch=-1 (scratch)");
    c.window = 20;
    run_case("window 20, 64x48x12 + 20x20x12", c, {&r6448, &r2020}, "kzch=-1 (scratch)");
    run_case("window 20, mixed layers (off)", c, {&r6448, &r2440}, "kzch=-1 (scratch)", false);
    run_case("window 20, fits LDS (off)", c, small, "kzch=-3", false);
    c.guide_cost = 50;
    run_case("window 20 with guide_cost (off)", c, {&r6448}, "kzch=-2", false);
    c = config(); c.block_threads = 512;
    run_case("block_threads 512", c, small, "kzch=-3");
    run_case("block_threads 512, 64x48x12", c, {&r6448}, "kzch=-1 (scratch)", false);
    c = config(); c.dial_mult = 5; c.path_cap = 17; c.debug_round_cap = 3; c.auto_reset = 1; c.max_route_count = 4; c.via_cost = 777; c.drc_cost = 3; c.drc_unit = 100;
    run_case("dial_mult, path_cap, round cap, costs", c, {&r4040}, "kzch=-3");
    // ---- batch sizes: the sweeps for the full rewrite from 4096 envs ------------------------------------------------------------------
    run_case("64 envs", config(64), small, "kzch=-3", false);
    run_case("4096 envs", config(4096), small, "kzch=-3");
    run_case("8200 envs", config(8200), small, "kzch=-3", false);
    run_case("4096 envs, odd N (no sweeps)", config(4096), {&r753, &a662}, "kzch=-3", false);
    c = config(4096); c.block_threads = 256;
    run_case("4096 envs, block_threads (no sweeps)", c, small, "kzch=-3", false);
    c = config(4096); c.router = XR_ROUTER_DIAL;
    run_case("4096 envs, router DIAL (no sweeps)", c, small, "kzch=-3", false);

    // ---- every refusal --------------------------------------------------------------------------------------------------------------
    {
        printf("case bad argument [rc=-1]\n");
        xr_batch* h = nullptr;
        c = config();
        check(xr_batch_create(&c, &h) == XR_OK, "create");
        xr_region_desc d = a662.desc();
        int32_t rc = xr_batch_load_regions(h, &d, 0, nullptr);
        printf("  load rc=%d error=\"%s\"\n", rc, xr_last_error());
        rc = xr_batch_load_regions(h, nullptr, 1, nullptr);
        printf("  load rc=%d error=\"%s\"\n", rc, xr_last_error());
        rc = xr_batch_load_regions(nullptr, &d, 1, nullptr);
        printf("  load rc=%d error=\"%s\"\n", rc, xr_last_error());
        g_reached["rc=-1"]++;
        xr_batch_destroy(h);
    }
    Reg bad = a662;
    bad.Z = 33;
    run_case("33 layers", config(), {&bad}, "rc=-5");
    bad = a662; bad.X = 0;
    run_case("dim_x 0", config(), {&bad}, "rc=-5");
    bad = Reg{}; bad.X = 32768; bad.Y = 32768; bad.Z = 2;       // (refused before any array is read)
    run_case("2^31 nodes", config(), {&bad}, "rc=-5");
    {
        printf("case null array [rc=-1]\n");
        xr_batch* h = nullptr;
        c = config();
        check(xr_batch_create(&c, &h) == XR_OK, "create");
        xr_region_desc d[2] = {a662.desc(), b662.desc()};
        d[1].layer_dir_host = nullptr;
        const int32_t rc = xr_batch_load_regions(h, d, 2, nullptr);
        printf("  load rc=%d error=\"%s\"\n", rc, xr_last_error());
        check(rc == XR_ERR_INVALID, "null array refused");
        xr_batch_destroy(h);
    }
    bad = a662; bad.K = XR_MAX_NETS + 1;
    run_case("n_nets above the limit", config(), {&bad}, "rc=-5");
    bad = a662; bad.K = -1;
    run_case("n_nets negative", config(), {&a662, &bad}, "rc=-5");
    bad = a662; bad.xs[0] = -(1 << 30) - 1;
    run_case("xs outside +-2^30", config(), {&bad}, "rc=-5");
    bad = a662; bad.ys[5] = (1 << 30) + 1;
    run_case("ys outside +-2^30", config(), {&bad}, "rc=-5");
    bad = a662; bad.xs[3] = bad.xs[2];
    run_case("xs not increasing", config(), {&bad}, "rc=-1");
    bad = a662; bad.ys[1] = bad.ys[0] - 1;
    run_case("ys not increasing", config(), {&bad}, "rc=-1");
    bad = a662; bad.nodes[7] = rec(XR_TYPE_ACCESS, bad.K + 1, 1);
    run_case("ACCESS node of a net beyond n_nets", config(), {&bad}, "rc=-5");
    bad = a662; bad.nodes[7] = rec(XR_TYPE_ACCESS, 0, 1);
    run_case("ACCESS node of net 0", config(), {&bad}, "rc=-5");
    bad = gen(20, 20, 20, 2, 1);
    for (int f = 0; f < 200; f++) bad.nodes[f] = rec(XR_TYPE_ACCESS, 1, 1 + f % 3);
    run_case("200 access points of one net", config(), {&a662, &bad}, "rc=-5");
    bad = a662; bad.K = 16000;
    run_case("16000 nets (LDS id list)", config(), {&bad}, "rc=-5");
    bad = gen(21, 300, 300, 1, 2, 400, 380, 1);
    run_case("90000 worklist items of one kind", config(), {&bad}, "rc=-5");
    bad = gen(22, 1, 30000, 1, 2, 400, 380, 1);
    run_case("edge tables beyond the LDS", config(), {&bad}, "rc=-5");
    // (the last refusal, XR_ROUTER_DIAL beyond the frontier router's limits, cannot be reached through the ABI: it needs a region of
    //  more than 1023 x 1024 nodes, and the worklist limit above refuses every region of more than 786432)

    // ---- the allocation limit at every size, each followed by an unlimited reload; then reloads that change the router form ---------
    {
        xr_batch* h = nullptr;
        c = config(64);
        check(xr_batch_create(&c, &h) == XR_OK, "create");
        const std::vector<const Reg*> limited{&a662};       // (64 slots of one 6x6x2 region: the limits below stop the load at five different buffers)
        for (int64_t lim : {0, 8, 64, 200, 512, 1024, 2048, 4096, 16384}) {
            printf("case allocation limit %lld [rc=-2]\n", (long long)lim);
            xr_stub_alloc_limit = lim;
            const int32_t rc = load_traced(h, limited, false);
            check(rc == XR_ERR_NOMEM, "the limited load runs out of memory");
            g_reached["rc=-2"]++;
            xr_stub_alloc_limit = -1;
            printf("case reload after limit %lld [kzch=-3]\n", (long long)lim);
            check(load_traced(h, limited, false) == XR_OK && g_seen.kzch == -3, "the unlimited reload succeeds");
        }
        printf("case reload: 64x48x12 over 6x6x2 [kzch=-1 (scratch)]\n");
        check(load_traced(h, {&r6448}, true) == XR_OK && g_seen.kzch == -1 && !g_seen.lds, "reload to the scratch form");
        printf("case reload: refused regions over a loaded batch [rc=-5]\n");
        bad = a662; bad.Z = 33;
        check(load_traced(h, {&bad}, false) == XR_ERR_RANGE, "refused reload");
        printf("case reload: 6x6x2 again [kzch=-3]\n");
        check(load_traced(h, small, true) == XR_OK && g_seen.kzch == -3, "reload to the LDS form");
        printf("case reload: 65536 nodes, guides kept out [kzch=-1 (scratch)]\n");
        check(load_traced(h, {&big}, false, false) == XR_OK && g_seen.kzch == -1, "reload to the scratch form");
        xr_batch_destroy(h);
        check(xr_stub_alloc_live == 0, "no device buffer outlives the batch");
    }

    printf("reached:\n");
    for (const auto& kv : g_reached) printf("  %-20s %d\n", kv.first.c_str(), kv.second);
    for (const char* need : {"kzch=9", "kzch=12", "kzch=0", "kzch=-1 (LDS)", "kzch=-1 (scratch)", "kzch=-2", "kzch=-3", "kzch=-4", "window", "sweep_full", "stream_ok=false"})
        if (!g_reached.count(need)) { printf("NOT REACHED: %s\n", need); g_failures++; }
    if (g_failures) printf("LOAD_TRACE_FAILED %d\n", g_failures);
    else printf("LOAD_TRACE_OK\n");
    range_cases();
    if (g_failures) printf("LOAD_TRACE_FAILED %d\n", g_failures);
    else printf("LOAD_TRACE_OK\n");
    return g_failures ? 1 : 0;
}
