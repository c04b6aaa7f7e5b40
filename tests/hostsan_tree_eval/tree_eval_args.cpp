// tests/hostsan_tree_eval/tree_eval_args.cpp — TEST INFRASTRUCTURE (see ../hostsan/hip/hip_runtime.h).
//
// Drives xr_batch_tree_open, xr_batch_tree_leaves and xr_batch_tree_backup of the product's host side (csrc/xr_batch.cpp, built with ASan +
// UBSan against the host-memory HIP stand-in) through every refusal include/xroute_hip.h documents that is decidable without a device —
// on batches with and without env groups, of the HBM-scratch forms and with stream_per_region, with fixed and with randomised arguments —
// and checks the code AND the message of each.  The stand-in links no tree launcher, so a valid open must answer XR_ERR_STATE ("not
// linked") after validating, without allocating or launching, and no session ever opens: valid leaves and backup calls must answer
// XR_ERR_STATE for the call order.  The stand-in's live-allocation and launch counters must not move on any call of this program.  Runs
// as a program of its own (no preload); ends with TREE_EVAL_ARGS_OK, no leak and nothing on stderr.
#include "../hostsan/args_common.h"

#include <cmath>
#include <limits>

namespace {

const double kNan = std::numeric_limits<double>::quiet_NaN(), kInf = std::numeric_limits<double>::infinity();

struct Open {
    int32_t group = -1, n_par = 2, node_cap = 64, max_sims = 8, k_cap = 64;
    double c_init = 1.25, c_base = 19652.0;
    bool prior = false;
};
struct Leaves {
    int32_t group = -1, region_base = 0;
    int64_t row_bytes = 4096;
    bool rows = true, out = true, ret = true, paths = true, leaf = true, misaligned = false;
};
struct Backup {
    int32_t group = -1;
    bool value = true, prior = false, visits = true, values = true, info = true, best = true, returns = true;
};

// what include/xroute_hip.h documents, in the order the entry points check
Expect expected(const Open& a, bool loaded, int n_groups, int rows, int k_max, bool scratch_form) {
    if (!loaded) return {XR_ERR_STATE, "load regions first"};
    if (a.group < -1 || a.group >= n_groups) return {XR_ERR_INVALID, "group"};
    if (!std::isfinite(a.c_init)) return {XR_ERR_INVALID, "c_init"};
    if (!(std::isfinite(a.c_base) && a.c_base > 0.0)) return {XR_ERR_INVALID, "c_base"};
    if (a.n_par < 1 || a.n_par > XR_PEEK_MAX) return {XR_ERR_RANGE, "n_par"};
    if (a.max_sims < a.n_par || a.max_sims > XR_TREE_MAX_SIMS) return {XR_ERR_RANGE, "max_sims"};
    if (a.node_cap < 1) return {XR_ERR_RANGE, "node_cap"};
    if (a.k_cap < k_max) return {XR_ERR_RANGE, "k_cap"};
    if (scratch_form) return {XR_ERR_RANGE, "HBM scratch"};
    if ((int64_t)rows * a.n_par >= ((int64_t)1 << 31)) return {XR_ERR_RANGE, "31 bits"};
    return {XR_ERR_STATE, "not linked"};
}

Expect expected(const Leaves& a, bool loaded, int n_groups, int64_t need, bool scratch_form) {
    if (!a.rows || !a.out) return {XR_ERR_INVALID, "null argument"};
    if (a.misaligned || a.row_bytes % 8 != 0) return {XR_ERR_INVALID, "8-byte aligned"};
    if (!loaded) return {XR_ERR_STATE, "load regions first"};
    if (a.group < -1 || a.group >= n_groups) return {XR_ERR_INVALID, "group"};
    if (a.row_bytes < need) return {XR_ERR_RANGE, "row_bytes"};
    if (scratch_form) return {XR_ERR_RANGE, "HBM scratch"};
    return {XR_ERR_STATE, "no open session"};          // (no session ever opens here)
}

Expect expected(const Backup& a, bool loaded, int n_groups) {
    if (!a.value || !a.visits || !a.values || !a.info) return {XR_ERR_INVALID, "null argument"};
    if (!loaded) return {XR_ERR_STATE, "load regions first"};
    if (a.group < -1 || a.group >= n_groups) return {XR_ERR_INVALID, "group"};
    return {XR_ERR_STATE, "no pending leaves"};
}

// stand-ins for the device buffers: never touched (nothing launches), but real memory
std::vector<int32_t> g_i32(8192);
std::vector<double> g_f64(1024);
std::vector<float> g_f32(1024);
alignas(16) uint8_t g_rows[8192 + 16];

void call(xr_batch* h, const Open& a, const Expect& want, const std::string& what) {
    const int64_t live = xr_stub_alloc_live, launches = xr_stub_launches;
    const int32_t rc = xr_batch_tree_open(h, a.group, a.n_par, a.node_cap, a.c_init, a.c_base, a.max_sims, a.prior ? g_f32.data() : nullptr, a.k_cap, nullptr);
    verdict("xr_batch_tree_open", rc, want, what, live, launches);
}

void call(xr_batch* h, const Leaves& a, const Expect& want, const std::string& what) {
    const int64_t live = xr_stub_alloc_live, launches = xr_stub_launches;
    const int32_t rc = xr_batch_tree_leaves(h, a.group, a.rows ? g_rows + (a.misaligned ? 4 : 0) : nullptr, a.row_bytes, a.region_base, a.out ? g_i32.data() : nullptr,
                                            a.ret ? g_f64.data() : nullptr, a.paths ? g_i32.data() + 4096 : nullptr, a.leaf ? g_i32.data() + 6144 : nullptr, nullptr);
    verdict("xr_batch_tree_leaves", rc, want, what, live, launches);
}

void call(xr_batch* h, const Backup& a, const Expect& want, const std::string& what) {
    const int64_t live = xr_stub_alloc_live, launches = xr_stub_launches;
    const int32_t rc = xr_batch_tree_backup(h, a.group, a.value ? g_f64.data() : nullptr, a.prior ? g_f32.data() : nullptr, a.visits ? g_i32.data() : nullptr,
                                            a.values ? g_f64.data() + 256 : nullptr, a.info ? g_i32.data() + 1024 : nullptr, a.best ? g_i32.data() + 2048 : nullptr,
                                            a.best ? g_f64.data() + 512 : nullptr, a.returns ? g_f64.data() + 768 : nullptr, nullptr);
    verdict("xr_batch_tree_backup", rc, want, what, live, launches);
}

Batch make(const char* name, int n_envs, const std::vector<const Reg*>& regs, int force_scratch, int per_region, const std::vector<int32_t>& bounds) {
    return make(name, n_envs, regs, force_scratch, per_region, bounds, [&](Batch& B) {
        call(B.h, Open{}, expected(Open{}, false, 1, n_envs, 0, false), std::string(name) + " open before the load");
        call(B.h, Leaves{}, expected(Leaves{}, false, 1, 0, false), std::string(name) + " leaves before the load");
        call(B.h, Backup{}, expected(Backup{}, false, 1), std::string(name) + " backup before the load");
    });
}

// every refusal once, by name, then randomised arguments
void drive(const char* name, Batch& B, Lcg& rng, int random_calls) {
    auto open = [&](Open a, const char* what) { call(B.h, a, expected(a, true, B.n_groups, B.rows(a.group), B.k_max, B.scratch_form), std::string(name) + " " + what); };
    auto leaves = [&](Leaves a, const char* what) { call(B.h, a, expected(a, true, B.n_groups, B.need, B.scratch_form), std::string(name) + " " + what); };
    auto backup = [&](Backup a, const char* what) { call(B.h, a, expected(a, true, B.n_groups), std::string(name) + " " + what); };
    Open a;
    open(a, "valid, defaults");
    a = Open{}; a.prior = true; open(a, "with a root prior");
    a = Open{}; a.group = -2; open(a, "group -2");
    a = Open{}; a.group = B.n_groups; open(a, "group n_groups");
    a = Open{}; a.group = B.n_groups - 1; open(a, "last group");
    a = Open{}; a.c_init = kNan; open(a, "c_init NaN");
    a = Open{}; a.c_init = kInf; open(a, "c_init inf");
    a = Open{}; a.c_init = -2.0; open(a, "c_init negative is a number");
    a = Open{}; a.c_base = 0.0; open(a, "c_base 0");
    a = Open{}; a.c_base = -1.0; open(a, "c_base -1");
    a = Open{}; a.c_base = kNan; open(a, "c_base NaN");
    a = Open{}; a.n_par = 0; open(a, "n_par 0");
    a = Open{}; a.n_par = -3; open(a, "n_par -3");
    a = Open{}; a.n_par = XR_PEEK_MAX; a.max_sims = XR_PEEK_MAX; open(a, "n_par at the limit");
    a = Open{}; a.n_par = XR_PEEK_MAX + 1; a.max_sims = XR_PEEK_MAX + 1; open(a, "n_par above the limit");
    a = Open{}; a.max_sims = 1; open(a, "max_sims below n_par");
    a = Open{}; a.max_sims = 2; open(a, "max_sims = n_par");
    a = Open{}; a.max_sims = XR_TREE_MAX_SIMS; open(a, "max_sims at the limit");
    a = Open{}; a.max_sims = XR_TREE_MAX_SIMS + 1; open(a, "max_sims above the limit");
    a = Open{}; a.node_cap = 0; open(a, "node_cap 0");
    a = Open{}; a.node_cap = 1; open(a, "node_cap 1");
    a = Open{}; a.k_cap = B.k_max - 1; open(a, "k_cap below k_max");
    a = Open{}; a.k_cap = B.k_max; open(a, "k_cap = k_max");
    Leaves l;
    leaves(l, "valid, before any open");
    l = Leaves{}; l.rows = false; leaves(l, "null rows_out_dev");
    l = Leaves{}; l.out = false; leaves(l, "null out_dev");
    l = Leaves{}; l.ret = l.paths = l.leaf = false; leaves(l, "optional outputs null");
    l = Leaves{}; l.misaligned = true; leaves(l, "rows_out_dev off by 4");
    l = Leaves{}; l.row_bytes = B.need + 4; leaves(l, "row_bytes not a multiple of 8");
    l = Leaves{}; l.row_bytes = B.need - 8; leaves(l, "row_bytes below the state row");
    l = Leaves{}; l.row_bytes = B.need; leaves(l, "row_bytes exactly the state row");
    l = Leaves{}; l.group = -2; leaves(l, "group -2");
    l = Leaves{}; l.group = B.n_groups; leaves(l, "group n_groups");
    l = Leaves{}; l.group = B.n_groups - 1; leaves(l, "last group");
    Backup k;
    backup(k, "valid, without leaves");
    k = Backup{}; k.value = false; backup(k, "null value_dev");
    k = Backup{}; k.visits = false; backup(k, "null visits_out_dev");
    k = Backup{}; k.values = false; backup(k, "null value_out_dev");
    k = Backup{}; k.info = false; backup(k, "null info_out_dev");
    k = Backup{}; k.best = k.returns = false; k.prior = true; backup(k, "optional arguments the other way round");
    k = Backup{}; k.group = -2; backup(k, "group -2");
    k = Backup{}; k.group = B.n_groups; backup(k, "group n_groups");
    k = Backup{}; k.group = B.n_groups - 1; backup(k, "last group");
    for (int i = 0; i < random_calls; i++) {
        Open r;
        r.group = rng.between(-3, B.n_groups + 1);
        r.n_par = rng.below(4) ? rng.between(1, 9) : (rng.below(2) ? rng.between(-3, 0) : rng.between(XR_PEEK_MAX - 1, XR_PEEK_MAX + 2));
        r.max_sims = rng.below(4) ? r.n_par + rng.between(-1, 40) : rng.between(XR_TREE_MAX_SIMS - 1, XR_TREE_MAX_SIMS + 2);
        r.node_cap = rng.below(4) ? rng.between(1, 500) : rng.between(-2, 0);
        r.k_cap = rng.between(B.k_max - 2, B.k_max + 2);
        const double ci[] = {1.25, 0.0, -1.0, kNan, kInf, -kInf}, cb[] = {19652.0, 1.0, 1e-9, 0.0, -5.0, kNan, kInf};
        r.c_init = ci[rng.below(3) ? 0 : rng.below(6)];
        r.c_base = cb[rng.below(3) ? 0 : rng.below(7)];
        r.prior = rng.below(2);
        open(r, "random");
        Leaves q;
        q.group = rng.between(-3, B.n_groups + 1);
        q.row_bytes = rng.below(3) ? 8 * rng.between(1, 512) : rng.between(0, 4096);
        q.region_base = rng.between(-5, 5);
        q.rows = rng.below(16) != 0; q.out = rng.below(16) != 0; q.ret = rng.below(2); q.paths = rng.below(2); q.leaf = rng.below(2);
        q.misaligned = rng.below(8) == 0;
        leaves(q, "random");
        Backup w;
        w.group = rng.between(-3, B.n_groups + 1);
        w.value = rng.below(16) != 0; w.visits = rng.below(16) != 0; w.values = rng.below(16) != 0; w.info = rng.below(16) != 0;
        w.prior = rng.below(2); w.best = rng.below(2); w.returns = rng.below(2);
        backup(w, "random");
    }
}

}  // namespace

int main() {
    const Reg a(6, 6, 3), b(7, 5, 5);
    Lcg rng{0x7EE6};
    {
        // a null batch, with and without the rest
        call(nullptr, Open{}, {XR_ERR_INVALID, "null argument"}, "null batch");
        Leaves l;
        call(nullptr, l, {XR_ERR_INVALID, "null argument"}, "null batch");
        l.out = false;
        call(nullptr, l, {XR_ERR_INVALID, "null argument"}, "null batch and out_dev");
        Backup k;
        call(nullptr, k, {XR_ERR_INVALID, "null argument"}, "null batch");
        k.info = false;
        call(nullptr, k, {XR_ERR_INVALID, "null argument"}, "null batch and info_out_dev");
    }
    struct Case { const char* name; int n_envs, scratch, per_region; std::vector<int32_t> bounds; };
    const Case cases[] = {{"whole batch", 6, 0, 0, {}}, {"three groups", 9, 0, 0, {0, 2, 5, 9}}, {"one group set", 4, 0, 0, {0, 4}},
                          {"force_scratch_field", 6, 1, 0, {}}, {"force_scratch_field, groups", 6, 1, 0, {0, 3, 6}}, {"stream_per_region", 5, 0, 1, {}}};
    for (const Case& c : cases) {
        Batch B = make(c.name, c.n_envs, {&a, &b}, c.scratch, c.per_region, c.bounds);
        drive(c.name, B, rng, 300);
        xr_batch_destroy(B.h);
        check(xr_stub_alloc_live == 0, std::string(c.name) + ": no device buffer outlives the batch");
    }
    {
        // rows x n_par beyond 31 bits: 2^19 slots x 4096 lanes (one group of the two is small enough)
        const Reg tiny(2, 2, 1);
        const int n = 1 << 19;
        Batch B = make("2^19 slots", n, {&tiny}, 0, 0, {0, n - 1, n});
        Open r;
        r.n_par = XR_PEEK_MAX; r.max_sims = XR_PEEK_MAX;
        call(B.h, r, {XR_ERR_RANGE, "31 bits"}, "2^19 rows x 4096");
        r.group = 0;
        call(B.h, r, {XR_ERR_STATE, "not linked"}, "2^19 - 1 rows x 4096");
        xr_batch_destroy(B.h);
        check(xr_stub_alloc_live == 0, "2^19 slots: no device buffer outlives the batch");
    }
    check(xr_stub_launches > 0, "the loads launched their kernels through the stand-in (the counters are live)");
    return finish("TREE_EVAL_ARGS");
}
