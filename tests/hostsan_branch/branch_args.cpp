// tests/hostsan_branch/branch_args.cpp — TEST INFRASTRUCTURE (see ../hostsan/hip/hip_runtime.h).
//
// Drives xr_batch_branch of the product's host side (csrc/xr_batch.cpp, built with ASan + UBSan against the host-memory HIP stand-in)
// through every refusal include/xroute_hip.h documents — on batches with and without env groups, of the HBM-scratch forms and with
// stream_per_region, with fixed and with randomised group indices — and checks the code AND the message of each.  Around every call the
// stand-in batch's arrays (every selector xr_batch_fetch knows; the stand-in's device memory is host memory) are snapshotted: every error
// path must leave them byte-identical.  The stand-in links no branch launcher, so a valid call must answer XR_ERR_STATE ("not linked")
// after validating, without allocating or launching: the stand-in's live-allocation and launch counters must not move on any call of
// this program.  Runs as a program of its own (no preload); ends with BRANCH_ARGS_OK, no leak and nothing on stderr.
#include "../hostsan/args_common.h"

#include <algorithm>

namespace {

// what include/xroute_hip.h documents, in the order the entry point checks
Expect expected(bool batch, bool parent, bool loaded, int group, int n_groups) {
    if (!batch || !parent) return {XR_ERR_INVALID, "null argument"};
    if (!loaded) return {XR_ERR_STATE, "load regions first"};
    if (group < -1 || group >= n_groups) return {XR_ERR_INVALID, "group"};
    return {XR_ERR_STATE, "not linked"};
}

// every array xr_batch_fetch returns, as bytes (empty before the load: fetch refuses then)
std::vector<uint8_t> snapshot(const Batch& B) {
    std::vector<uint8_t> all;
    if (!B.loaded) return all;
    const size_t n = (size_t)B.n_envs;
    const size_t row = std::max<size_t>({(size_t)B.n_max * 2, (size_t)B.path_cap * 4, (size_t)B.legal_words * 8, (size_t)64});
    std::vector<uint8_t> buf(n * row + 64);
    for (int what = 0; what <= 20; what++) {
        memset(buf.data(), 0, buf.size());
        const int32_t rc = xr_batch_fetch(B.h, what, buf.data(), buf.size(), nullptr);
        check(rc == XR_OK, std::string("fetch of selector ") + std::to_string(what) + ": " + xr_last_error());
        all.insert(all.end(), buf.begin(), buf.end());
    }
    return all;
}

std::vector<int32_t> g_parent(1 << 12, 0);

void call(const Batch& B, int group, bool parent, const std::string& what) {
    const Expect want = expected(B.h != nullptr, parent, B.loaded, group, B.n_groups);
    const std::vector<uint8_t> before = snapshot(B);
    const int64_t live = xr_stub_alloc_live, launches = xr_stub_launches;
    const int32_t rc = xr_batch_branch(B.h, group, parent ? g_parent.data() : nullptr, nullptr);
    g_calls++;
    const std::string msg = xr_last_error();
    char buf[512];
    snprintf(buf, sizeof buf, "%s: group %d parent %d -> rc %d \"%s\", expected %d \"...%s...\"", what.c_str(), group, (int)parent, rc, msg.c_str(), want.code,
             want.msg);
    check(rc == want.code && strstr(msg.c_str(), "xr_batch_branch") && strstr(msg.c_str(), want.msg), buf);
    check(xr_stub_alloc_live == live && xr_stub_launches == launches, std::string("allocated or launched: ") + buf);
    check(snapshot(B) == before, std::string("the batch's arrays changed: ") + buf);
}

Batch make(const char* name, int n_envs, const std::vector<const Reg*>& regs, int force_scratch, int per_region, const std::vector<int32_t>& bounds) {
    return make(name, n_envs, regs, force_scratch, per_region, bounds, [&](Batch& B) {
        call(B, -1, true, std::string(name) + " before the load");
        call(B, -1, false, std::string(name) + " before the load, null parent");
        call(B, 5, true, std::string(name) + " before the load, bad group");
    });
}

// every refusal once, by name, then randomised group indices (far out of range too)
void drive(const char* name, const Batch& B, Lcg& rng, int random_calls) {
    const std::string n(name);
    call(B, -1, true, n + " valid, whole batch");
    call(B, -1, false, n + " null parent_dev");
    call(B, 0, false, n + " null parent_dev, group 0");
    call(B, 0, true, n + " group 0");
    call(B, B.n_groups - 1, true, n + " last group");
    call(B, B.n_groups, true, n + " group n_groups");
    call(B, -2, true, n + " group -2");
    call(B, XR_MAX_GROUPS, true, n + " group XR_MAX_GROUPS");
    call(B, XR_MAX_GROUPS + 1, true, n + " group XR_MAX_GROUPS + 1");
    call(B, 0x7FFFFFFF, true, n + " group INT32_MAX");
    call(B, (int32_t)0x80000000u, true, n + " group INT32_MIN");
    for (int i = 0; i < random_calls; i++) {
        const int pick = rng.below(8);
        const int group = pick < 5 ? rng.between(-3, B.n_groups + 2) : (pick == 5 ? rng.between(60, 70) : (int)rng.next() * (rng.below(2) ? 1 : -1));
        for (int32_t& p : g_parent) p = (int32_t)rng.next() - (1 << 30);          // (never read: nothing launches)
        call(B, group, rng.below(8) != 0, n + " random");
    }
}

}  // namespace

int main() {
    const Reg a(6, 6, 3), b(7, 5, 5);
    Lcg rng{0xB7A2C4};
    {
        Batch none;          // a null batch, with and without the map
        call(none, -1, true, "null batch");
        call(none, 0, false, "null batch and parent_dev");
    }
    struct Case { const char* name; int n_envs, scratch, per_region; std::vector<int32_t> bounds; };
    const Case cases[] = {{"whole batch", 6, 0, 0, {}}, {"three groups", 9, 0, 0, {0, 2, 5, 9}}, {"one group set", 4, 0, 0, {0, 4}},
                          {"force_scratch_field", 6, 1, 0, {}}, {"force_scratch_field, groups", 6, 1, 0, {0, 3, 6}}, {"stream_per_region", 5, 0, 1, {}}};
    for (const Case& c : cases) {
        Batch B = make(c.name, c.n_envs, {&a, &b}, c.scratch, c.per_region, c.bounds);
        drive(c.name, B, rng, 120);
        xr_batch_destroy(B.h);
        check(xr_stub_alloc_live == 0, std::string(c.name) + ": no device buffer outlives the batch");
    }
    check(xr_stub_launches > 0, "the loads launched their kernels through the stand-in (the counters are live)");
    return finish("BRANCH_ARGS");
}
