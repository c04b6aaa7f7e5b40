// tests/hostsan_tree/tree_args.cpp — TEST INFRASTRUCTURE (see ../hostsan/hip/hip_runtime.h).
//
// Drives xr_batch_tree_search and xr_tree_exploration_table of the product's host side (csrc/xr_batch.cpp, built with ASan + UBSan
// against the host-memory HIP stand-in) through every refusal include/xroute_hip.h documents — on batches with and without env groups, of
// the HBM-scratch forms and with stream_per_region, with fixed and with randomised arguments — and checks the code AND the message of
// each.  The stand-in links no tree launcher, so a valid call must answer XR_ERR_STATE ("not linked") after validating, without
// allocating or launching: the stand-in's live-allocation and launch counters must not move on any call of this program.  The table
// function is checked against its formula.  Runs as a program of its own (no preload); ends with TREE_ARGS_OK, no leak and nothing on
// stderr.
#include "../hostsan/args_common.h"

#include <cmath>
#include <limits>

namespace {

const double kNan = std::numeric_limits<double>::quiet_NaN(), kInf = std::numeric_limits<double>::infinity();

struct Args {
    int32_t group = -1, n_waves = 2, n_par = 2, node_cap = 64, k_cap = 64;
    double c_init = 1.25, c_base = 19652.0;
    bool prior = false, visits = true, value = true, info = true, best = true, trace = false;
};

// what include/xroute_hip.h documents, in the order the entry point checks
Expect expected(const Args& a, bool loaded, int n_groups, int rows, int k_max, bool scratch_form) {
    if (!a.visits || !a.value || !a.info) return {XR_ERR_INVALID, "null argument"};
    if (!loaded) return {XR_ERR_STATE, "load regions first"};
    if (a.group < -1 || a.group >= n_groups) return {XR_ERR_INVALID, "group"};
    if (a.n_waves < 1) return {XR_ERR_INVALID, "n_waves"};
    if (a.n_par < 1) return {XR_ERR_INVALID, "n_par"};
    if (!std::isfinite(a.c_init)) return {XR_ERR_INVALID, "c_init"};
    if (!(std::isfinite(a.c_base) && a.c_base > 0.0)) return {XR_ERR_INVALID, "c_base"};
    if (a.n_par > XR_ROLLOUT_MAX) return {XR_ERR_RANGE, "n_par"};
    if ((int64_t)a.n_waves * a.n_par > XR_TREE_MAX_SIMS) return {XR_ERR_RANGE, "simulations"};
    if (a.node_cap < 1) return {XR_ERR_RANGE, "node_cap"};
    if (a.k_cap < k_max) return {XR_ERR_RANGE, "k_cap"};
    if (scratch_form) return {XR_ERR_RANGE, "HBM scratch"};
    if ((int64_t)rows * a.n_par >= ((int64_t)1 << 31)) return {XR_ERR_RANGE, "31 bits"};
    return {XR_ERR_STATE, "not linked"};
}

// stand-ins for the device buffers: never touched (nothing launches), but real memory
std::vector<int32_t> g_visits(64), g_info(64), g_order(64), g_paths(64);
std::vector<double> g_value(64), g_best(8), g_returns(8);
std::vector<float> g_prior(64);

void call(xr_batch* b, const Args& a, const Expect& want, const std::string& what) {
    const int64_t live = xr_stub_alloc_live, launches = xr_stub_launches;
    const int32_t rc = xr_batch_tree_search(b, a.group, a.n_waves, a.n_par, 0x1234567ULL * (uint64_t)(g_calls + 1), a.prior ? g_prior.data() : nullptr, a.node_cap,
                                            a.c_init, a.c_base, a.visits ? g_visits.data() : nullptr, a.value ? g_value.data() : nullptr, a.k_cap,
                                            a.info ? g_info.data() : nullptr, a.best ? g_order.data() : nullptr, a.best ? g_best.data() : nullptr,
                                            a.trace ? g_paths.data() : nullptr, a.trace ? g_returns.data() : nullptr, nullptr);
    g_calls++;
    const char* msg = xr_last_error();
    char buf[512];
    snprintf(buf, sizeof buf, "%s: group %d waves %d par %d cap %d k_cap %d c %g/%g -> rc %d \"%s\", expected %d \"...%s...\"", what.c_str(), a.group, a.n_waves,
             a.n_par, a.node_cap, a.k_cap, a.c_init, a.c_base, rc, msg, want.code, want.msg);
    check(rc == want.code && strstr(msg, "xr_batch_tree_search") && strstr(msg, want.msg), buf);
    check(xr_stub_alloc_live == live && xr_stub_launches == launches, std::string("allocated or launched: ") + buf);
}

Batch make(const char* name, int n_envs, const std::vector<const Reg*>& regs, int force_scratch, int per_region, const std::vector<int32_t>& bounds) {
    return make(name, n_envs, regs, force_scratch, per_region, bounds, [&](Batch& B) {
        Args a;
        call(B.h, a, expected(a, false, 1, n_envs, 0, false), std::string(name) + " before the load");
    });
}

// every refusal once, by name, then randomised arguments
void drive(const char* name, Batch& B, Lcg& rng, int random_calls) {
    auto run = [&](Args a, const char* what) { call(B.h, a, expected(a, true, B.n_groups, B.rows(a.group < -1 || a.group >= B.n_groups ? -1 : a.group), B.k_max, B.scratch_form),
                                                     std::string(name) + " " + what); };
    Args a;
    run(a, "valid, defaults");
    a = Args{}; a.visits = false; run(a, "null visits_out_dev");
    a = Args{}; a.value = false; run(a, "null value_out_dev");
    a = Args{}; a.info = false; run(a, "null info_out_dev");
    a = Args{}; a.group = -2; run(a, "group -2");
    a = Args{}; a.group = B.n_groups; run(a, "group n_groups");
    a = Args{}; a.group = B.n_groups - 1; run(a, "last group");
    a = Args{}; a.n_waves = 0; run(a, "n_waves 0");
    a = Args{}; a.n_par = 0; run(a, "n_par 0");
    a = Args{}; a.n_par = -3; run(a, "n_par -3");
    a = Args{}; a.c_init = kNan; run(a, "c_init NaN");
    a = Args{}; a.c_init = kInf; run(a, "c_init inf");
    a = Args{}; a.c_init = -2.0; run(a, "c_init negative is a number");
    a = Args{}; a.c_base = 0.0; run(a, "c_base 0");
    a = Args{}; a.c_base = -1.0; run(a, "c_base -1");
    a = Args{}; a.c_base = kNan; run(a, "c_base NaN");
    a = Args{}; a.n_par = XR_ROLLOUT_MAX + 1; run(a, "n_par above the limit");
    a = Args{}; a.n_par = XR_ROLLOUT_MAX; a.n_waves = 16; run(a, "65536 simulations");
    a = Args{}; a.n_par = XR_ROLLOUT_MAX; a.n_waves = 17; run(a, "above 65536 simulations");
    a = Args{}; a.n_par = 1; a.n_waves = XR_TREE_MAX_SIMS + 1; run(a, "65537 waves of one");
    a = Args{}; a.node_cap = 0; run(a, "node_cap 0");
    a = Args{}; a.node_cap = 1; run(a, "node_cap 1");
    a = Args{}; a.k_cap = B.k_max - 1; run(a, "k_cap below k_max");
    a = Args{}; a.k_cap = B.k_max; run(a, "k_cap = k_max");
    a = Args{}; a.best = false; a.trace = true; a.prior = true; run(a, "optional outputs the other way round");
    for (int i = 0; i < random_calls; i++) {
        Args r;
        r.group = rng.between(-3, B.n_groups + 1);
        r.n_waves = rng.below(4) ? rng.between(1, 9) : rng.between(-2, 0);
        r.n_par = rng.below(4) ? rng.between(1, 9) : (rng.below(2) ? rng.between(-3, 0) : rng.between(XR_ROLLOUT_MAX - 1, XR_ROLLOUT_MAX + 2));
        if (!rng.below(8)) r.n_waves = rng.between(15, 18);
        r.node_cap = rng.below(4) ? rng.between(1, 500) : rng.between(-2, 0);
        r.k_cap = rng.between(B.k_max - 2, B.k_max + 2);
        const double ci[] = {1.25, 0.0, -1.0, kNan, kInf, -kInf}, cb[] = {19652.0, 1.0, 1e-9, 0.0, -5.0, kNan, kInf};
        r.c_init = ci[rng.below(3) ? 0 : rng.below(6)];
        r.c_base = cb[rng.below(3) ? 0 : rng.below(7)];
        r.prior = rng.below(2); r.best = rng.below(2); r.trace = rng.below(2);
        r.visits = rng.below(16) != 0; r.value = rng.below(16) != 0; r.info = rng.below(16) != 0;
        run(r, "random");
    }
}

void tables() {
    std::vector<double> t(1002, -1.0);
    check(xr_tree_exploration_table(1.25, 19652.0, 1000, t.data()) == XR_OK, "table: defaults");
    check(t[0] == 0.0 && t[1001] == -1.0, "table: E[0] == 0, nothing past n");
    for (int n = 1; n <= 1000; n++) {
        const double want = (std::log(((double)n + 19652.0 + 1.0) / 19652.0) + 1.25) * std::sqrt((double)n);
        check(t[n] == want && t[n] > t[n - 1], "table: entry " + std::to_string(n));
    }
    double one = -1.0;
    check(xr_tree_exploration_table(0.5, 10.0, 0, &one) == XR_OK && one == 0.0, "table: n = 0");
    check(xr_tree_exploration_table(1.25, 19652.0, 4, nullptr) == XR_ERR_INVALID && strstr(xr_last_error(), "xr_tree_exploration_table"), "table: null out");
    check(xr_tree_exploration_table(1.25, 19652.0, -1, t.data()) == XR_ERR_INVALID, "table: n < 0");
    check(xr_tree_exploration_table(kNan, 19652.0, 4, t.data()) == XR_ERR_INVALID, "table: c_init NaN");
    check(xr_tree_exploration_table(1.25, 0.0, 4, t.data()) == XR_ERR_INVALID, "table: c_base 0");
    check(xr_tree_exploration_table(1.25, kInf, 4, t.data()) == XR_ERR_INVALID, "table: c_base inf");
}

}  // namespace

int main() {
    const Reg a(6, 6, 3), b(7, 5, 5);
    Lcg rng{0x7EE5};
    tables();
    {
        Args n;          // a null batch, with and without the rest
        call(nullptr, n, {XR_ERR_INVALID, "null argument"}, "null batch");
        n.info = false;
        call(nullptr, n, {XR_ERR_INVALID, "null argument"}, "null batch and info_out_dev");
    }
    struct Case { const char* name; int n_envs, scratch, per_region; std::vector<int32_t> bounds; };
    const Case cases[] = {{"whole batch", 6, 0, 0, {}}, {"three groups", 9, 0, 0, {0, 2, 5, 9}}, {"one group set", 4, 0, 0, {0, 4}},
                          {"force_scratch_field", 6, 1, 0, {}}, {"force_scratch_field, groups", 6, 1, 0, {0, 3, 6}}, {"stream_per_region", 5, 0, 1, {}}};
    for (const Case& c : cases) {
        Batch B = make(c.name, c.n_envs, {&a, &b}, c.scratch, c.per_region, c.bounds);
        drive(c.name, B, rng, 400);
        xr_batch_destroy(B.h);
        check(xr_stub_alloc_live == 0, std::string(c.name) + ": no device buffer outlives the batch");
    }
    {
        // rows x n_par beyond 31 bits: 2^19 slots x 4096 lanes (one group of the two is small enough)
        const Reg tiny(2, 2, 1);
        const int n = 1 << 19;
        Batch B = make("2^19 slots", n, {&tiny}, 0, 0, {0, n - 1, n});
        Args r;
        r.n_par = XR_ROLLOUT_MAX; r.n_waves = 1;
        call(B.h, r, {XR_ERR_RANGE, "31 bits"}, "2^19 rows x 4096");
        r.group = 0;
        call(B.h, r, {XR_ERR_STATE, "not linked"}, "2^19 - 1 rows x 4096");
        xr_batch_destroy(B.h);
        check(xr_stub_alloc_live == 0, "2^19 slots: no device buffer outlives the batch");
    }
    check(xr_stub_launches > 0, "the loads launched their kernels through the stand-in (the counters are live)");
    return finish("TREE_ARGS");
}
