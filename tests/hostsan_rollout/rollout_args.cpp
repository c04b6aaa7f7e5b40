// tests/hostsan_rollout/rollout_args.cpp — TEST INFRASTRUCTURE (see ../hostsan/hip/hip_runtime.h).
//
// Drives xr_batch_rollout of the product's host side (csrc/xr_batch.cpp, built with ASan + UBSan against the host-memory HIP stand-in)
// through every refusal include/xroute_hip.h documents — on batches with and without env groups, of the HBM-scratch forms and with
// stream_per_region, with fixed and with randomised arguments — and checks the code AND the message of each.  The stand-in links no
// rollout launcher, so a valid call must answer XR_ERR_STATE ("not linked") after validating, without allocating or launching: the
// stand-in's live-allocation and launch counters must not move on any call of this program.  Runs as a program of its own (no preload);
// ends with ROLLOUT_ARGS_OK, no leak and nothing on stderr.
#include "../hostsan/args_common.h"

namespace {

struct Args {
    int32_t group = -1, n_rollouts = 1, policy = XR_ROLLOUT_RANDOM, prefix_stride = 0, max_plies = 0, k_cap = 0;
    bool prefix = false, out = true, ret = true, hash = true, order = false;
};

// what include/xroute_hip.h documents, in the order the entry point checks
Expect expected(const Args& a, bool loaded, int n_groups, int rows, int k_max, bool scratch_form) {
    if (!a.out) return {XR_ERR_INVALID, "null argument"};
    if (!loaded) return {XR_ERR_STATE, "load regions first"};
    if (a.group < -1 || a.group >= n_groups) return {XR_ERR_INVALID, "group"};
    if (a.policy != XR_ROLLOUT_STOP && a.policy != XR_ROLLOUT_RANDOM) return {XR_ERR_INVALID, "unknown policy"};
    if (a.prefix && a.prefix_stride < 1) return {XR_ERR_INVALID, "prefix_stride"};
    if (a.max_plies < 0) return {XR_ERR_INVALID, "max_plies"};
    if (a.n_rollouts < 1 || a.n_rollouts > XR_ROLLOUT_MAX) return {XR_ERR_RANGE, "n_rollouts"};
    if (a.order && a.k_cap < k_max) return {XR_ERR_RANGE, "k_cap"};
    if (scratch_form) return {XR_ERR_RANGE, "HBM scratch"};
    if ((int64_t)rows * a.n_rollouts >= ((int64_t)1 << 31)) return {XR_ERR_RANGE, "31 bits"};
    return {XR_ERR_STATE, "not linked"};
}

// stand-ins for the device buffers: never touched (nothing launches), but real memory of a plausible size
std::vector<int32_t> g_out(64), g_order(64), g_prefix(64);
std::vector<double> g_ret(8);
std::vector<uint64_t> g_hash(8);

void call(xr_batch* b, const Args& a, const Expect& want, const std::string& what) {
    const int64_t live = xr_stub_alloc_live, launches = xr_stub_launches;
    const int32_t rc = xr_batch_rollout(b, a.group, a.n_rollouts, a.policy, 0x1234567ULL * (uint64_t)(g_calls + 1), a.prefix ? g_prefix.data() : nullptr,
                                        a.prefix_stride, a.max_plies, a.out ? g_out.data() : nullptr, a.ret ? g_ret.data() : nullptr,
                                        a.hash ? g_hash.data() : nullptr, a.order ? g_order.data() : nullptr, a.k_cap, nullptr);
    g_calls++;
    const char* msg = xr_last_error();
    char buf[512];
    snprintf(buf, sizeof buf, "%s: group %d R %d policy %d prefix %d/%d max_plies %d order %d/%d -> rc %d \"%s\", expected %d \"...%s...\"", what.c_str(), a.group,
             a.n_rollouts, a.policy, (int)a.prefix, a.prefix_stride, a.max_plies, (int)a.order, a.k_cap, rc, msg, want.code, want.msg);
    check(rc == want.code && strstr(msg, "xr_batch_rollout") && strstr(msg, want.msg), buf);
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
    a = Args{}; a.out = false; run(a, "null out_dev");
    a = Args{}; a.group = -2; run(a, "group -2");
    a = Args{}; a.group = B.n_groups; run(a, "group n_groups");
    a = Args{}; a.group = B.n_groups - 1; run(a, "last group");
    a = Args{}; a.policy = 2; run(a, "policy 2");
    a = Args{}; a.policy = -1; run(a, "policy -1");
    a = Args{}; a.policy = XR_ROLLOUT_STOP; run(a, "policy STOP");
    a = Args{}; a.prefix = true; a.prefix_stride = 0; run(a, "prefix with stride 0");
    a = Args{}; a.prefix = true; a.prefix_stride = -3; run(a, "prefix with stride -3");
    a = Args{}; a.prefix = true; a.prefix_stride = 4; run(a, "prefix with stride 4");
    a = Args{}; a.prefix_stride = -3; run(a, "no prefix, stride ignored");
    a = Args{}; a.max_plies = -1; run(a, "max_plies -1");
    a = Args{}; a.max_plies = 3; run(a, "max_plies 3");
    a = Args{}; a.n_rollouts = 0; run(a, "n_rollouts 0");
    a = Args{}; a.n_rollouts = -7; run(a, "n_rollouts -7");
    a = Args{}; a.n_rollouts = XR_ROLLOUT_MAX + 1; run(a, "n_rollouts above the limit");
    a = Args{}; a.n_rollouts = XR_ROLLOUT_MAX; run(a, "n_rollouts at the limit");
    a = Args{}; a.order = true; a.k_cap = B.k_max - 1; run(a, "k_cap below k_max with order_out");
    a = Args{}; a.order = true; a.k_cap = B.k_max; run(a, "k_cap = k_max with order_out");
    a = Args{}; a.k_cap = -5; run(a, "k_cap ignored without order_out");
    a = Args{}; a.ret = false; a.hash = false; run(a, "optional outputs null");
    for (int i = 0; i < random_calls; i++) {
        Args r;
        r.group = rng.between(-3, B.n_groups + 1);
        r.n_rollouts = rng.below(4) ? rng.between(1, 9) : (rng.below(2) ? rng.between(-3, 0) : rng.between(XR_ROLLOUT_MAX - 1, XR_ROLLOUT_MAX + 2));
        r.policy = rng.below(4) ? rng.below(2) : rng.between(-2, 4);
        r.prefix = rng.below(2);
        r.prefix_stride = rng.below(4) ? rng.between(1, 6) : rng.between(-2, 0);
        r.max_plies = rng.below(4) ? rng.between(0, 9) : rng.between(-4, -1);
        r.order = rng.below(2);
        r.k_cap = rng.between(B.k_max - 2, B.k_max + 2);
        r.out = rng.below(16) != 0; r.ret = rng.below(2); r.hash = rng.below(2);
        run(r, "random");
    }
}

}  // namespace

int main() {
    const Reg a(6, 6, 3), b(7, 5, 5);
    Lcg rng{0x5EED};
    {
        Args n;          // a null batch, with and without the rest
        call(nullptr, n, {XR_ERR_INVALID, "null argument"}, "null batch");
        n.out = false;
        call(nullptr, n, {XR_ERR_INVALID, "null argument"}, "null batch and out_dev");
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
        // rows x n_rollouts beyond 31 bits: 2^19 slots x 4096 rollouts (one group of the two is small enough)
        const Reg tiny(2, 2, 1);
        const int n = 1 << 19;
        Batch B = make("2^19 slots", n, {&tiny}, 0, 0, {0, n - 1, n});
        Args r;
        r.n_rollouts = XR_ROLLOUT_MAX;
        call(B.h, r, {XR_ERR_RANGE, "31 bits"}, "2^19 rows x 4096");
        r.group = 0;
        call(B.h, r, {XR_ERR_STATE, "not linked"}, "2^19 - 1 rows x 4096");
        r.group = -1; r.n_rollouts = XR_ROLLOUT_MAX - 1;
        call(B.h, r, {XR_ERR_STATE, "not linked"}, "2^19 rows x 4095");
        xr_batch_destroy(B.h);
        check(xr_stub_alloc_live == 0, "2^19 slots: no device buffer outlives the batch");
    }
    check(xr_stub_launches > 0, "the loads launched their kernels through the stand-in (the counters are live)");
    return finish("ROLLOUT_ARGS");
}
