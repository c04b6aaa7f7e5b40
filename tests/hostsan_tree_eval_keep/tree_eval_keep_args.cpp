// tests/hostsan_tree_eval_keep/tree_eval_keep_args.cpp — TEST INFRASTRUCTURE (see ../hostsan/hip/hip_runtime.h).
//
// Drives xr_batch_tree_reopen of the product's host side (csrc/xr_batch.cpp, built with ASan + UBSan against the host-memory HIP stand-in)
// (1) through every refusal include/xroute_hip.h documents that is decidable without a device — with fixed and with randomised arguments,
// on batches with and without env groups, of the HBM-scratch forms and with stream_per_region — checking the code AND the message of each,
// and that a refused call neither allocates nor launches; and (2) through the call sequences that decide what a reopen keeps: reopen /
// leaves / backup / reopen, an open in between, leaves without a backup, a changed n_par / node_cap / k_cap, set_groups in between, a
// group beside the whole batch, a refused table.  The search launchers are ../hostsan/stub_launch_search.cpp's; the launcher of the reopen
// kernel is this file's own and records what it is handed.  Part (2) prints a trace — which half is old and which is new, whether `played`
// reaches the launcher or NULL does, the table's length, the carve offsets — that tests/test_tree_eval_keep_host.py compares with
// tree_eval_keep_args.expected; no address is printed.  Runs as a program of its own (no preload); its last line is
// TREE_EVAL_KEEP_ARGS_OK, with no leak and nothing on stderr.
#include "../hostsan/args_common.h"
#include "../hostsan/stub_launch_search.h"

#include <cmath>
#include <limits>

#include "../../xroute_env_amd/csrc/xr_device.h"

namespace {
const double kNan = std::numeric_limits<double>::quiet_NaN(), kInf = std::numeric_limits<double>::infinity();
bool g_trace = false;
const uint8_t* g_base = nullptr;          // the pool of the last reopen launch: the lower of its two halves
int g_reopens = 0, g_played_seen = 0;

long long off(const void* p) { return p ? (long long)(static_cast<const uint8_t*>(p) - g_base) : -1; }
}  // namespace

// the launcher of xr_tree_eval_reopen_kernel: nothing runs; what it is handed goes to the trace
extern "C" hipError_t xr_launch_tree_eval_reopen(const XrBatchDev* src, const XrTreeEvalDev* t, const XrTreeKeepDev* k, const float* root_prior, int rows,
                                                 hipStream_t) {
    xr_stub_launches++;
    g_reopens++;
    if (k->played) g_played_seen++;
    const uint8_t* const a = reinterpret_cast<const uint8_t*>(t->nodes);
    const uint8_t* const b = reinterpret_cast<const uint8_t*>(k->old_nodes);
    g_base = a < b ? a : b;
    check(k->key_legal == t->legal, "the key's legal words are the session's snapshot");
    check(t->e_max == XR_TREE_MAX_SIMS, "a keyed session's table runs to XR_TREE_MAX_SIMS");
    check(a != b, "two halves");
    if (!g_trace) return hipSuccess;
    printf("  launch tree_eval_reopen rows=%d env_lo=%d src.env_base=%d new=half%d old=half%d played=%s kept_out=%s root_prior=%s has_prior=%d n_add=%d e_max=%d\n", rows,
           t->env_lo, src->env_base, a == g_base ? 0 : 1, b == g_base ? 0 : 1, k->played ? "caller" : "NULL", k->kept_out ? "caller" : "NULL", root_prior ? "caller" : "NULL",
           t->has_prior, k->n_add, t->e_max);
    printf("    carve nodes=%lld old_nodes=%lld rs=%lld prefix=%lld ret=%lld leaf=%lld best_order=%lld legal=%lld nlegal=%lld prior=%lld key=%lld | node_cap=%d n_par=%d k_cap=%d "
           "legal_words=%d\n", off(t->nodes), off(k->old_nodes), off(t->rs), off(t->prefix), off(t->ret), off(t->leaf), off(t->best_order), off(t->legal), off(t->nlegal),
           off(t->prior), off(k->key), t->node_cap, t->n_par, t->k_cap, t->legal_words);
    return hipSuccess;
}

namespace {

struct Reopen {
    int32_t group = -1, n_par = 2, node_cap = 64, max_sims = 8, k_cap = 64;
    double c_init = 1.25, c_base = 19652.0;
    bool prior = false, played = true, kept = true;
};

// what include/xroute_hip.h documents, in the order xr_batch_tree_open checks; a valid call succeeds here (the launchers are linked)
Expect expected(const Reopen& a, bool loaded, int n_groups, int rows, int k_max, bool scratch_form) {
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
    return {XR_OK, ""};
}

std::vector<int32_t> g_played(1 << 20), g_kept(1 << 21), g_i32(1 << 16);
std::vector<float> g_f32(1 << 12);
std::vector<double> g_f64(1 << 12);
alignas(16) uint8_t g_rows[1 << 18];

int32_t reopen(xr_batch* h, const Reopen& a) {
    return xr_batch_tree_reopen(h, a.group, a.played ? g_played.data() : nullptr, a.n_par, a.node_cap, a.c_init, a.c_base, a.max_sims, a.prior ? g_f32.data() : nullptr, a.k_cap,
                                a.kept ? g_kept.data() : nullptr, nullptr);
}

void call(xr_batch* h, const Reopen& a, const Expect& want, const std::string& what) {
    const int64_t live = xr_stub_alloc_live, launches = xr_stub_launches;
    const int32_t rc = reopen(h, a);
    if (want.code != XR_OK) { verdict("xr_batch_tree_reopen", rc, want, what, live, launches); return; }
    g_calls++;
    check(rc == XR_OK, "xr_batch_tree_reopen " + what + ": a valid call must succeed: " + xr_last_error());
    check(xr_stub_launches == launches + 1, "xr_batch_tree_reopen " + what + ": one launch");
}

void drive(const char* name, Batch& B, Lcg& rng, int random_calls) {
    auto go = [&](Reopen a, const char* what) {
        if (a.k_cap == 64) a.k_cap = B.k_max;
        call(B.h, a, expected(a, true, B.n_groups, B.rows(a.group), B.k_max, B.scratch_form), std::string(name) + " " + what);
    };
    Reopen a;
    go(a, "valid, defaults");
    a = Reopen{}; a.prior = true; a.played = false; a.kept = false; go(a, "a root prior, no played, no kept_out");
    a = Reopen{}; a.group = -2; go(a, "group -2");
    a = Reopen{}; a.group = B.n_groups; go(a, "group n_groups");
    a = Reopen{}; a.group = B.n_groups - 1; go(a, "last group");
    a = Reopen{}; a.c_init = kNan; go(a, "c_init NaN");
    a = Reopen{}; a.c_init = kInf; go(a, "c_init inf");
    a = Reopen{}; a.c_init = -2.0; go(a, "c_init negative is a number");
    a = Reopen{}; a.c_base = 0.0; go(a, "c_base 0");
    a = Reopen{}; a.c_base = -1.0; go(a, "c_base -1");
    a = Reopen{}; a.c_base = kNan; go(a, "c_base NaN");
    a = Reopen{}; a.n_par = 0; go(a, "n_par 0");
    a = Reopen{}; a.n_par = -3; go(a, "n_par -3");
    a = Reopen{}; a.n_par = XR_PEEK_MAX + 1; a.max_sims = XR_PEEK_MAX + 1; go(a, "n_par above the limit");
    a = Reopen{}; a.max_sims = 1; go(a, "max_sims below n_par");
    a = Reopen{}; a.max_sims = 2; go(a, "max_sims = n_par");
    a = Reopen{}; a.max_sims = XR_TREE_MAX_SIMS; go(a, "max_sims at the limit");
    a = Reopen{}; a.max_sims = XR_TREE_MAX_SIMS + 1; go(a, "max_sims above the limit");
    a = Reopen{}; a.node_cap = 0; go(a, "node_cap 0");
    a = Reopen{}; a.node_cap = 1; go(a, "node_cap 1");
    a = Reopen{}; a.k_cap = B.k_max - 1; go(a, "k_cap below k_max");
    a = Reopen{}; a.k_cap = B.k_max + 3; go(a, "k_cap above k_max");
    for (int i = 0; i < random_calls; i++) {
        Reopen r;
        r.group = rng.between(-3, B.n_groups + 1);
        r.n_par = rng.below(4) ? rng.between(1, 9) : (rng.below(2) ? rng.between(-3, 0) : rng.between(XR_PEEK_MAX, XR_PEEK_MAX + 2));
        r.max_sims = rng.below(4) ? r.n_par + rng.between(-1, 40) : rng.between(XR_TREE_MAX_SIMS - 1, XR_TREE_MAX_SIMS + 2);
        r.node_cap = rng.below(4) ? rng.between(1, 200) : rng.between(-2, 0);
        r.k_cap = rng.between(B.k_max - 2, B.k_max + 2);
        if (r.k_cap == 64) r.k_cap = 65;
        const double ci[] = {1.25, 0.0, -1.0, kNan, kInf, -kInf}, cb[] = {19652.0, 1.0, 1e-9, 0.0, -5.0, kNan, kInf};
        r.c_init = ci[rng.below(3) ? 0 : rng.below(6)];
        r.c_base = cb[rng.below(3) ? 0 : rng.below(7)];
        r.prior = rng.below(2); r.played = rng.below(2); r.kept = rng.below(2);
        go(r, "random");
    }
}

// ---- part 2: the call sequences, traced -----------------------------------------------------------------------------------------------
void on_malloc(size_t bytes) {
    if (g_trace) printf("  hipMalloc %zu\n", bytes);
}

void on_async(const char* what, const void*, int kind, size_t bytes) {
    if (g_trace && kind == 1) printf("  %s host-to-device %zu bytes (a table of %zu entries)\n", what, bytes, bytes / sizeof(double));
}

void on_launch(const char* launcher, const XrStubArg* a, int n) {
    if (!g_trace) return;
    printf("  launch %s", launcher);
    for (int i = 0; i < n; i++) {
        if (!strcmp(a[i].name, "t.nodes") && strncmp(launcher, "tree_eval", 9) == 0) printf(" on half%d", a[i].p == g_base ? 0 : 1);
        if (!strcmp(a[i].name, "t.e_max") || !strcmp(a[i].name, "sims")) printf(" %s=%lld", a[i].name, (long long)a[i].i);
    }
    printf("\n");
}

struct Seq {
    Batch& B;
    int32_t said(const char* fn, int32_t rc) {
        g_calls++;
        printf("%s -> rc %d%s%s\n", fn, rc, rc ? ": " : "", rc ? xr_last_error() : "");
        return rc;
    }
    int32_t reopen(Reopen a) {
        if (a.k_cap == 64) a.k_cap = B.k_max;
        printf("reopen group %d par %d node_cap %d k_cap %s%d max_sims %d c_init %g prior %d played %d\n", a.group, a.n_par, a.node_cap, "k_max+", a.k_cap - B.k_max, a.max_sims,
               a.c_init, (int)a.prior, (int)a.played);
        return said("xr_batch_tree_reopen", ::reopen(B.h, a));
    }
    int32_t open(int32_t group = -1) {
        printf("open group %d\n", group);
        return said("xr_batch_tree_open", xr_batch_tree_open(B.h, group, 2, 64, 1.25, 19652.0, 8, nullptr, B.k_max, nullptr));
    }
    int32_t leaves(int32_t group = -1) {
        return said("xr_batch_tree_leaves", xr_batch_tree_leaves(B.h, group, g_rows, B.need, 0, g_i32.data(), g_f64.data(), nullptr, nullptr, nullptr));
    }
    int32_t backup(int32_t group = -1) {
        return said("xr_batch_tree_backup", xr_batch_tree_backup(B.h, group, g_f64.data(), nullptr, g_i32.data(), g_f64.data() + 1024, g_i32.data() + 4096, nullptr, nullptr,
                                                                 nullptr, nullptr));
    }
};

void sequences() {
    const Reg a(6, 5, 3), b(7, 4, 2);
    Batch B = make("sequences", 5, {&a, &b}, 0, 0, {0, 2, 5}, [](Batch&) {});
    printf("sequences: n_envs 5 groups 2 k_max %d legal_words %d row_bytes %lld\n", B.k_max, B.legal_words, (long long)B.need);
    g_trace = true;
    Seq s{B};
    const Reopen r;
    auto expect_played = [&](bool reaches, const char* what) {
        static int seen = 0;
        check((g_played_seen - seen == 1) == reaches, what);
        seen = g_played_seen;
    };
    printf("# the first reopen of a pool: nothing to keep\n");
    s.reopen(r); expect_played(false, "the first reopen gets NULL");
    s.leaves(); s.backup();
    printf("# reopen / leaves / backup / reopen: played reaches the kernel, the halves swap\n");
    s.reopen(r); expect_played(true, "the second reopen gets played");
    s.leaves(); s.backup();
    s.reopen(r); expect_played(true, "the third reopen gets played");
    printf("# max_sims, the knobs and the prior may differ (other knobs: another table)\n");
    { Reopen q; q.max_sims = 6; q.c_init = 2.5; q.prior = true; s.reopen(q); expect_played(true, "other knobs keep the tree"); }
    printf("# played NULL: a fresh session that leaves a keyed tree behind\n");
    { Reopen q; q.played = false; s.reopen(q); expect_played(false, "played NULL"); }
    s.reopen(r); expect_played(true, "after a fresh keyed session");
    printf("# an open in between: its session is not keyed\n");
    s.open(); s.leaves(); s.backup();
    s.reopen(r); expect_played(false, "after an open session");
    s.reopen(r); expect_played(true, "keyed again");
    printf("# leaves without a backup: pending visits forfeit the tree\n");
    s.leaves();
    s.reopen(r); expect_played(false, "after an abandoned wave");
    s.leaves(); s.leaves(); s.backup(); s.backup();
    s.reopen(r); expect_played(true, "after a refused second leaves and a refused second backup");
    printf("# a wave that would pass max_sims is refused and the tree is kept\n");
    { Reopen q; q.max_sims = 2; s.reopen(q); expect_played(true, "max_sims 2"); s.leaves(); s.backup(); s.leaves(); s.reopen(r); expect_played(true, "after a refused wave"); }
    printf("# a changed n_par, node_cap, k_cap: every row is rebuilt, then kept again under the new shape\n");
    { Reopen q; q.n_par = 3; s.reopen(q); expect_played(false, "n_par 3"); s.reopen(q); expect_played(true, "n_par 3 again"); }
    { Reopen q; q.n_par = 3; q.node_cap = 65; s.reopen(q); expect_played(false, "node_cap 65"); s.reopen(q); expect_played(true, "node_cap 65 again"); }
    { Reopen q; q.n_par = 3; q.node_cap = 65; q.k_cap = B.k_max + 1; s.reopen(q); expect_played(false, "k_cap + 1"); s.reopen(q); expect_played(true, "k_cap + 1 again"); }
    s.reopen(r); expect_played(false, "back to the first shape: a smaller carve of the same allocation");
    printf("# a group's pool beside the whole batch's\n");
    { Reopen q; q.group = 1; s.reopen(q); expect_played(false, "group 1, first"); s.leaves(1); s.backup(1); s.reopen(q); expect_played(true, "group 1, second"); }
    s.reopen(r); expect_played(true, "the whole batch's tree is still there");
    printf("# set_groups in between: every row is rebuilt\n");
    const int32_t bounds[] = {0, 2, 5};
    check(xr_batch_set_groups(B.h, bounds, 2) == XR_OK, "set_groups");
    s.reopen(r); expect_played(false, "after set_groups");
    { Reopen q; q.group = 1; s.reopen(q); expect_played(false, "group 1 after set_groups"); }
    s.reopen(r); expect_played(true, "keyed again after set_groups");
    printf("# a refused argument leaves the session alone; a refused table ends it\n");
    { Reopen q; q.node_cap = 0; s.reopen(q); s.leaves(); s.backup(); s.reopen(r); expect_played(true, "after a refused argument"); }
    {
        Reopen q; q.c_base = 100.0;
        xr_stub_alloc_limit = 0;
        check(s.reopen(q) == XR_ERR_NOMEM, "the table of other knobs is refused");
        xr_stub_alloc_limit = -1;
        s.leaves();
        s.reopen(q); expect_played(false, "after a refused table");
    }
    g_trace = false;
    xr_batch_destroy(B.h);
    check(xr_stub_alloc_live == 0, "sequences: no device buffer outlives the batch");
    printf("destroy | live %lld B\n", (long long)xr_stub_alloc_live);
}

}  // namespace

int main() {
    xr_stub_malloc_hook = on_malloc;
    xr_stub_async_hook = on_async;
    xr_stub_search_hook = on_launch;
    const Reg a(6, 6, 3), b(7, 5, 5);
    Lcg rng{0x2EE7};
    {
        const int64_t live = xr_stub_alloc_live, launches = xr_stub_launches;
        verdict("xr_batch_tree_reopen", reopen(nullptr, Reopen{}), {XR_ERR_INVALID, "null argument"}, "null batch", live, launches);
    }
    struct Case { const char* name; int n_envs, scratch, per_region; std::vector<int32_t> bounds; };
    const Case cases[] = {{"whole batch", 6, 0, 0, {}}, {"three groups", 9, 0, 0, {0, 2, 5, 9}}, {"force_scratch_field", 6, 1, 0, {}},
                          {"force_scratch_field, groups", 6, 1, 0, {0, 3, 6}}, {"stream_per_region", 5, 0, 1, {}}};
    for (const Case& c : cases) {
        Batch B = make(c.name, c.n_envs, {&a, &b}, c.scratch, c.per_region, c.bounds, [&](Batch& B0) {
            const int64_t live = xr_stub_alloc_live, launches = xr_stub_launches;
            verdict("xr_batch_tree_reopen", reopen(B0.h, Reopen{}), {XR_ERR_STATE, "load regions first"}, std::string(c.name) + " before the load", live, launches);
        });
        drive(c.name, B, rng, 200);
        xr_batch_destroy(B.h);
        check(xr_stub_alloc_live == 0, std::string(c.name) + ": no device buffer outlives the batch");
    }
    {
        // rows x n_par beyond 31 bits: 2^19 slots x 4096 lanes (one group of the two is small enough)
        const Reg tiny(2, 2, 1);
        const int n = 1 << 19;
        Batch B = make("2^19 slots", n, {&tiny}, 0, 0, {0, n - 1, n}, [](Batch&) {});
        Reopen r;
        r.n_par = XR_PEEK_MAX; r.max_sims = XR_PEEK_MAX; r.k_cap = B.k_max; r.node_cap = 2;
        call(B.h, r, {XR_ERR_RANGE, "31 bits"}, "2^19 rows x 4096");
        xr_batch_destroy(B.h);
        check(xr_stub_alloc_live == 0, "2^19 slots: no device buffer outlives the batch");
    }
    check(g_reopens > 0, "valid calls reached the reopen launcher");
    sequences();
    return finish("TREE_EVAL_KEEP_ARGS");
}
