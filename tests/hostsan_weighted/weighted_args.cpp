// tests/hostsan_weighted/weighted_args.cpp — TEST INFRASTRUCTURE (see ../hostsan/hip/hip_runtime.h).
//
// Drives xr_batch_weighted_actions, xr_batch_rollout_weighted and xr_batch_tree_search_weighted of the product's host side
// (csrc/xr_batch.cpp, built with ASan + UBSan against the host-memory HIP stand-in) through every refusal include/xroute_hip.h documents —
// on batches with and without env groups, of the HBM-scratch forms and with stream_per_region, with fixed and with randomised arguments —
// and checks the code AND the message of each.  The stand-in links none of the launchers, so a valid call must answer XR_ERR_STATE
// ("not linked") after validating, without allocating or launching: the stand-in's live-allocation and launch counters must not move on
// any call of this program.  Runs as a program of its own (no preload); ends with WEIGHTED_ARGS_OK, no leak and nothing on stderr.
#include "../hostsan/args_common.h"

#include <cmath>
#include <limits>

namespace {

const double kNan = std::numeric_limits<double>::quiet_NaN(), kInf = std::numeric_limits<double>::infinity();

struct Ctx { bool loaded; int n_groups, rows, k_max; bool scratch_form; };

// stand-ins for the device buffers: never touched (nothing launches), but real memory
std::vector<int32_t> g_i32a(64), g_i32b(64), g_i32c(64), g_i32d(64), g_weights(64);
std::vector<double> g_f64a(64), g_f64b(8);
std::vector<uint64_t> g_hash(8);
std::vector<float> g_prior(64);

// ---- xr_batch_weighted_actions ------------------------------------------------------------------------------------------------------
struct ActArgs {
    int32_t group = -1, k_cap = 64;
    bool weights = true, actions = true;
};
Expect expected(const ActArgs& a, const Ctx& c) {
    if (!a.weights || !a.actions) return {XR_ERR_INVALID, "null argument"};
    if (!c.loaded) return {XR_ERR_STATE, "load regions first"};
    if (a.group < -1 || a.group >= c.n_groups) return {XR_ERR_INVALID, "group"};
    if (a.k_cap < c.k_max) return {XR_ERR_RANGE, "k_cap"};
    return {XR_ERR_STATE, "not linked"};
}
void call(xr_batch* b, const ActArgs& a, const Expect& want, const std::string& what) {
    const int64_t live = xr_stub_alloc_live, launches = xr_stub_launches;
    const int32_t rc = xr_batch_weighted_actions(b, a.group, a.weights ? g_weights.data() : nullptr, a.k_cap, a.actions ? g_i32a.data() : nullptr,
                                                 0x1234567ULL * (uint64_t)(g_calls + 1), nullptr);
    verdict("xr_batch_weighted_actions", rc, want, what + " group " + std::to_string(a.group) + " k_cap " + std::to_string(a.k_cap), live, launches);
}

// ---- xr_batch_rollout_weighted ------------------------------------------------------------------------------------------------------
struct RollArgs {
    int32_t group = -1, n_rollouts = 1, policy = XR_ROLLOUT_WEIGHTED, prefix_stride = 0, max_plies = 0, k_cap = 0, weights_k_cap = 64;
    bool prefix = false, out = true, ret = true, hash = true, order = false, weights = true;
};
Expect expected(const RollArgs& a, const Ctx& c) {
    if (!a.out) return {XR_ERR_INVALID, "null argument"};
    if (!c.loaded) return {XR_ERR_STATE, "load regions first"};
    if (a.group < -1 || a.group >= c.n_groups) return {XR_ERR_INVALID, "group"};
    if (a.policy != XR_ROLLOUT_STOP && a.policy != XR_ROLLOUT_RANDOM && a.policy != XR_ROLLOUT_WEIGHTED) return {XR_ERR_INVALID, "unknown policy"};
    const bool by_weights = a.policy == XR_ROLLOUT_WEIGHTED;
    if (by_weights && !a.weights) return {XR_ERR_INVALID, "null weights_dev"};
    if (a.prefix && a.prefix_stride < 1) return {XR_ERR_INVALID, "prefix_stride"};
    if (a.max_plies < 0) return {XR_ERR_INVALID, "max_plies"};
    if (a.n_rollouts < 1 || a.n_rollouts > XR_ROLLOUT_MAX) return {XR_ERR_RANGE, "n_rollouts"};
    if (a.order && a.k_cap < c.k_max) return {XR_ERR_RANGE, ": k_cap"};
    if (by_weights && a.weights_k_cap < c.k_max) return {XR_ERR_RANGE, "weights_k_cap"};
    if (c.scratch_form) return {XR_ERR_RANGE, "HBM scratch"};
    if ((int64_t)c.rows * a.n_rollouts >= ((int64_t)1 << 31)) return {XR_ERR_RANGE, "31 bits"};
    return {XR_ERR_STATE, "not linked"};
}
void call(xr_batch* b, const RollArgs& a, const Expect& want, const std::string& what) {
    const int64_t live = xr_stub_alloc_live, launches = xr_stub_launches;
    const int32_t rc = xr_batch_rollout_weighted(b, a.group, a.n_rollouts, a.policy, 0x1234567ULL * (uint64_t)(g_calls + 1), a.prefix ? g_i32c.data() : nullptr,
                                                 a.prefix_stride, a.max_plies, a.out ? g_i32a.data() : nullptr, a.ret ? g_f64a.data() : nullptr,
                                                 a.hash ? g_hash.data() : nullptr, a.order ? g_i32b.data() : nullptr, a.k_cap,
                                                 a.weights ? g_weights.data() : nullptr, a.weights_k_cap, nullptr);
    char buf[256];
    snprintf(buf, sizeof buf, "%s group %d R %d policy %d prefix %d/%d max_plies %d order %d/%d weights %d/%d", what.c_str(), a.group, a.n_rollouts, a.policy,
             (int)a.prefix, a.prefix_stride, a.max_plies, (int)a.order, a.k_cap, (int)a.weights, a.weights_k_cap);
    verdict("xr_batch_rollout_weighted", rc, want, buf, live, launches);
}

// ---- xr_batch_tree_search_weighted --------------------------------------------------------------------------------------------------
struct TreeArgs {
    int32_t group = -1, n_waves = 2, n_par = 2, node_cap = 64, k_cap = 64;
    double c_init = 1.25, c_base = 19652.0;
    bool prior = false, visits = true, value = true, info = true, best = true, trace = false, sim_weights = true;
};
Expect expected(const TreeArgs& a, const Ctx& c) {
    if (!a.visits || !a.value || !a.info) return {XR_ERR_INVALID, "null argument"};
    if (!c.loaded) return {XR_ERR_STATE, "load regions first"};
    if (a.group < -1 || a.group >= c.n_groups) return {XR_ERR_INVALID, "group"};
    if (a.n_waves < 1) return {XR_ERR_INVALID, "n_waves"};
    if (a.n_par < 1) return {XR_ERR_INVALID, "n_par"};
    if (!std::isfinite(a.c_init)) return {XR_ERR_INVALID, "c_init"};
    if (!(std::isfinite(a.c_base) && a.c_base > 0.0)) return {XR_ERR_INVALID, "c_base"};
    if (a.n_par > XR_ROLLOUT_MAX) return {XR_ERR_RANGE, "n_par"};
    if ((int64_t)a.n_waves * a.n_par > XR_TREE_MAX_SIMS) return {XR_ERR_RANGE, "simulations"};
    if (a.node_cap < 1) return {XR_ERR_RANGE, "node_cap"};
    if (a.k_cap < c.k_max) return {XR_ERR_RANGE, "k_cap"};
    if (c.scratch_form) return {XR_ERR_RANGE, "HBM scratch"};
    if ((int64_t)c.rows * a.n_par >= ((int64_t)1 << 31)) return {XR_ERR_RANGE, "31 bits"};
    return {XR_ERR_STATE, "not linked"};
}
void call(xr_batch* b, const TreeArgs& a, const Expect& want, const std::string& what) {
    const int64_t live = xr_stub_alloc_live, launches = xr_stub_launches;
    const int32_t rc = xr_batch_tree_search_weighted(b, a.group, a.n_waves, a.n_par, 0x1234567ULL * (uint64_t)(g_calls + 1), a.prior ? g_prior.data() : nullptr,
                                                     a.node_cap, a.c_init, a.c_base, a.visits ? g_i32a.data() : nullptr, a.value ? g_f64a.data() : nullptr,
                                                     a.k_cap, a.info ? g_i32b.data() : nullptr, a.best ? g_i32c.data() : nullptr,
                                                     a.best ? g_f64b.data() : nullptr, a.trace ? g_i32d.data() : nullptr, a.trace ? g_f64b.data() : nullptr,
                                                     a.sim_weights ? g_weights.data() : nullptr, nullptr);
    char buf[256];
    snprintf(buf, sizeof buf, "%s group %d waves %d par %d cap %d k_cap %d c %g/%g sim_weights %d", what.c_str(), a.group, a.n_waves, a.n_par, a.node_cap, a.k_cap,
             a.c_init, a.c_base, (int)a.sim_weights);
    verdict("xr_batch_tree_search_weighted", rc, want, buf, live, launches);
}

Ctx ctx(const Batch& B, int g) { return {true, B.n_groups, B.rows(g), B.k_max, B.scratch_form}; }

Batch make(const char* name, int n_envs, const std::vector<const Reg*>& regs, int force_scratch, int per_region, const std::vector<int32_t>& bounds) {
    return make(name, n_envs, regs, force_scratch, per_region, bounds, [&](Batch& B) {
        const Ctx before{false, 1, n_envs, 0, false};
        call(B.h, ActArgs{}, expected(ActArgs{}, before), std::string(name) + " before the load");
        call(B.h, RollArgs{}, expected(RollArgs{}, before), std::string(name) + " before the load");
        call(B.h, TreeArgs{}, expected(TreeArgs{}, before), std::string(name) + " before the load");
    });
}

// every refusal once, by name, then randomised arguments
void drive(const char* name, Batch& B, Lcg& rng, int random_calls) {
    auto run = [&](auto a, const char* what) { call(B.h, a, expected(a, ctx(B, a.group)), std::string(name) + " " + what); };
    {
        ActArgs a;
        run(a, "valid, defaults");
        a = ActArgs{}; a.weights = false; run(a, "null weights_dev");
        a = ActArgs{}; a.actions = false; run(a, "null actions_dev");
        a = ActArgs{}; a.group = -2; run(a, "group -2");
        a = ActArgs{}; a.group = B.n_groups; run(a, "group n_groups");
        a = ActArgs{}; a.group = B.n_groups - 1; run(a, "last group");
        a = ActArgs{}; a.k_cap = B.k_max - 1; run(a, "k_cap below k_max");
        a = ActArgs{}; a.k_cap = B.k_max; run(a, "k_cap = k_max");
        a = ActArgs{}; a.k_cap = -1; run(a, "k_cap -1");
    }
    {
        RollArgs a;
        run(a, "valid, defaults");
        a = RollArgs{}; a.out = false; run(a, "null out_dev");
        a = RollArgs{}; a.group = -2; run(a, "group -2");
        a = RollArgs{}; a.group = B.n_groups; run(a, "group n_groups");
        a = RollArgs{}; a.group = B.n_groups - 1; run(a, "last group");
        a = RollArgs{}; a.policy = 3; run(a, "policy 3");
        a = RollArgs{}; a.policy = -1; run(a, "policy -1");
        a = RollArgs{}; a.policy = XR_ROLLOUT_STOP; a.weights = false; run(a, "policy STOP, no weights");
        a = RollArgs{}; a.policy = XR_ROLLOUT_RANDOM; a.weights = false; a.weights_k_cap = -4; run(a, "policy RANDOM, no weights, weights_k_cap ignored");
        a = RollArgs{}; a.weights = false; run(a, "policy WEIGHTED, null weights_dev");
        a = RollArgs{}; a.weights_k_cap = B.k_max - 1; run(a, "weights_k_cap below k_max");
        a = RollArgs{}; a.weights_k_cap = B.k_max; run(a, "weights_k_cap = k_max");
        a = RollArgs{}; a.prefix = true; a.prefix_stride = 0; run(a, "prefix with stride 0");
        a = RollArgs{}; a.prefix = true; a.prefix_stride = 4; run(a, "prefix with stride 4");
        a = RollArgs{}; a.max_plies = -1; run(a, "max_plies -1");
        a = RollArgs{}; a.n_rollouts = 0; run(a, "n_rollouts 0");
        a = RollArgs{}; a.n_rollouts = XR_ROLLOUT_MAX + 1; run(a, "n_rollouts above the limit");
        a = RollArgs{}; a.n_rollouts = XR_ROLLOUT_MAX; run(a, "n_rollouts at the limit");
        a = RollArgs{}; a.order = true; a.k_cap = B.k_max - 1; run(a, "k_cap below k_max with order_out");
        a = RollArgs{}; a.order = true; a.k_cap = B.k_max; run(a, "k_cap = k_max with order_out");
        a = RollArgs{}; a.ret = false; a.hash = false; run(a, "optional outputs null");
    }
    {
        TreeArgs a;
        run(a, "valid, defaults");
        a = TreeArgs{}; a.sim_weights = false; run(a, "null sim_weights_dev is the plain search");
        a = TreeArgs{}; a.visits = false; run(a, "null visits_out_dev");
        a = TreeArgs{}; a.value = false; run(a, "null value_out_dev");
        a = TreeArgs{}; a.info = false; run(a, "null info_out_dev");
        a = TreeArgs{}; a.group = -2; run(a, "group -2");
        a = TreeArgs{}; a.group = B.n_groups; run(a, "group n_groups");
        a = TreeArgs{}; a.n_waves = 0; run(a, "n_waves 0");
        a = TreeArgs{}; a.n_par = 0; run(a, "n_par 0");
        a = TreeArgs{}; a.c_init = kNan; run(a, "c_init NaN");
        a = TreeArgs{}; a.c_base = 0.0; run(a, "c_base 0");
        a = TreeArgs{}; a.c_base = kInf; run(a, "c_base inf");
        a = TreeArgs{}; a.n_par = XR_ROLLOUT_MAX + 1; run(a, "n_par above the limit");
        a = TreeArgs{}; a.n_par = XR_ROLLOUT_MAX; a.n_waves = 17; run(a, "above 65536 simulations");
        a = TreeArgs{}; a.node_cap = 0; run(a, "node_cap 0");
        a = TreeArgs{}; a.k_cap = B.k_max - 1; run(a, "k_cap below k_max");
        a = TreeArgs{}; a.k_cap = B.k_max; run(a, "k_cap = k_max");
        a = TreeArgs{}; a.best = false; a.trace = true; a.prior = true; run(a, "optional outputs the other way round");
    }
    for (int i = 0; i < random_calls; i++) {
        ActArgs x;
        x.group = rng.between(-3, B.n_groups + 1);
        x.k_cap = rng.between(B.k_max - 2, B.k_max + 2);
        x.weights = rng.below(8) != 0; x.actions = rng.below(8) != 0;
        run(x, "random");
        RollArgs r;
        r.group = rng.between(-3, B.n_groups + 1);
        r.n_rollouts = rng.below(4) ? rng.between(1, 9) : (rng.below(2) ? rng.between(-3, 0) : rng.between(XR_ROLLOUT_MAX - 1, XR_ROLLOUT_MAX + 2));
        r.policy = rng.below(4) ? rng.below(3) : rng.between(-2, 5);
        r.prefix = rng.below(2);
        r.prefix_stride = rng.below(4) ? rng.between(1, 6) : rng.between(-2, 0);
        r.max_plies = rng.below(4) ? rng.between(0, 9) : rng.between(-4, -1);
        r.order = rng.below(2);
        r.k_cap = rng.between(B.k_max - 2, B.k_max + 2);
        r.weights = rng.below(4) != 0;
        r.weights_k_cap = rng.between(B.k_max - 2, B.k_max + 2);
        r.out = rng.below(16) != 0; r.ret = rng.below(2); r.hash = rng.below(2);
        run(r, "random");
        TreeArgs t;
        t.group = rng.between(-3, B.n_groups + 1);
        t.n_waves = rng.below(4) ? rng.between(1, 9) : rng.between(-2, 0);
        t.n_par = rng.below(4) ? rng.between(1, 9) : (rng.below(2) ? rng.between(-3, 0) : rng.between(XR_ROLLOUT_MAX - 1, XR_ROLLOUT_MAX + 2));
        if (!rng.below(8)) t.n_waves = rng.between(15, 18);
        t.node_cap = rng.below(4) ? rng.between(1, 500) : rng.between(-2, 0);
        t.k_cap = rng.between(B.k_max - 2, B.k_max + 2);
        const double ci[] = {1.25, 0.0, -1.0, kNan, kInf, -kInf}, cb[] = {19652.0, 1.0, 1e-9, 0.0, -5.0, kNan, kInf};
        t.c_init = ci[rng.below(3) ? 0 : rng.below(6)];
        t.c_base = cb[rng.below(3) ? 0 : rng.below(7)];
        t.prior = rng.below(2); t.best = rng.below(2); t.trace = rng.below(2); t.sim_weights = rng.below(4) != 0;
        t.visits = rng.below(16) != 0; t.value = rng.below(16) != 0; t.info = rng.below(16) != 0;
        run(t, "random");
    }
}

}  // namespace

int main() {
    const Reg a(6, 6, 3), b(7, 5, 5);
    Lcg rng{0x3E16};
    {
        // a null batch
        call(nullptr, ActArgs{}, {XR_ERR_INVALID, "null argument"}, "null batch");
        call(nullptr, RollArgs{}, {XR_ERR_INVALID, "null argument"}, "null batch");
        call(nullptr, TreeArgs{}, {XR_ERR_INVALID, "null argument"}, "null batch");
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
    check(xr_stub_launches > 0, "the loads launched their kernels through the stand-in (the counters are live)");
    return finish("WEIGHTED_ARGS");
}
