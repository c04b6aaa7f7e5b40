// tests/hostsan_peek/peek_args.cpp — TEST INFRASTRUCTURE (see ../hostsan/hip/hip_runtime.h).
//
// Drives xr_batch_peek of the product's host side (csrc/xr_batch.cpp, built with ASan + UBSan against the host-memory HIP stand-in)
// through every refusal include/xroute_hip.h documents — on batches with and without env groups, of the HBM-scratch forms and with
// stream_per_region, with fixed, hostile (INT32_MIN / INT32_MAX, misaligned pointers) and randomised arguments — and checks the code
// AND the message of each.  The stand-in links no peek launcher, so a valid call must answer XR_ERR_STATE ("not linked") after
// validating, without allocating or launching: the stand-in's live-allocation and launch counters must not move on any call of this
// program.  Runs as a program of its own (no preload); ends with PEEK_ARGS_OK, no leak and nothing on stderr.
#include "../hostsan/args_common.h"

#include <climits>

namespace {

// row_bytes < 0 in Args: "the batch's minimum plus row_extra"; rows_off: bytes added to the (8-byte aligned) row pointer
struct Args {
    int32_t group = -1, n_lines = 1, prefix_stride = 0, max_plies = 0, k_cap = 0, region_base = 0;
    int64_t row_bytes = -1, row_extra = 0;
    int rows_off = 0;
    bool prefix = false, rows = true, out = true, ret = true, hash = true, order = false;
};

// what include/xroute_hip.h documents, in the order the entry point checks
Expect expected(const Args& a, int64_t row_bytes, bool loaded, int n_groups, int rows, int k_max, int64_t need, bool scratch_form) {
    if (!a.rows || !a.out) return {XR_ERR_INVALID, "null argument"};
    if (a.rows_off % 8 != 0 || row_bytes % 8 != 0) return {XR_ERR_INVALID, "8-byte aligned"};
    if (!loaded) return {XR_ERR_STATE, "load regions first"};
    if (a.group < -1 || a.group >= n_groups) return {XR_ERR_INVALID, "group"};
    if (a.prefix && a.prefix_stride < 1) return {XR_ERR_INVALID, "prefix_stride"};
    if (a.max_plies < 0) return {XR_ERR_INVALID, "max_plies"};
    if (a.n_lines < 1 || a.n_lines > XR_PEEK_MAX) return {XR_ERR_RANGE, "n_lines"};
    if (row_bytes < need) return {XR_ERR_RANGE, "row_bytes"};
    if (a.order && a.k_cap < k_max) return {XR_ERR_RANGE, "k_cap"};
    if (scratch_form) return {XR_ERR_RANGE, "HBM scratch"};
    if ((int64_t)rows * a.n_lines >= ((int64_t)1 << 31)) return {XR_ERR_RANGE, "31 bits"};
    return {XR_ERR_STATE, "not linked"};
}

// stand-ins for the device buffers: never touched (nothing launches), but real memory of a plausible size
std::vector<int32_t> g_out(64), g_order(64), g_prefix(64);
std::vector<double> g_ret(8);
std::vector<uint64_t> g_hash(8), g_rows(64);

void call(const Batch& B, const Args& a, const std::string& what, const Expect* forced = nullptr) {
    const int64_t live = xr_stub_alloc_live, launches = xr_stub_launches;
    const int64_t rb = a.row_bytes >= 0 || a.row_extra == INT64_MIN ? a.row_bytes : B.need + a.row_extra;
    const Expect want = forced ? *forced : expected(a, rb, B.loaded, B.n_groups, B.rows(a.group), B.k_max, B.need, B.scratch_form);
    uint8_t* rows = a.rows ? reinterpret_cast<uint8_t*>(g_rows.data()) + a.rows_off : nullptr;
    const int32_t rc = xr_batch_peek(B.h, a.group, a.n_lines, a.prefix ? g_prefix.data() : nullptr, a.prefix_stride, a.max_plies, rows, rb, a.region_base,
                                     a.out ? g_out.data() : nullptr, a.ret ? g_ret.data() : nullptr, a.hash ? g_hash.data() : nullptr,
                                     a.order ? g_order.data() : nullptr, a.k_cap, nullptr);
    g_calls++;
    const char* msg = xr_last_error();
    char buf[640];
    snprintf(buf, sizeof buf, "%s: group %d L %d prefix %d/%d max_plies %d rows %d+%d row_bytes %lld order %d/%d -> rc %d \"%s\", expected %d \"...%s...\"",
             what.c_str(), a.group, a.n_lines, (int)a.prefix, a.prefix_stride, a.max_plies, (int)a.rows, a.rows_off, (long long)rb, (int)a.order, a.k_cap, rc, msg,
             want.code, want.msg);
    check(rc == want.code && strstr(msg, "xr_batch_peek") && strstr(msg, want.msg), buf);
    check(xr_stub_alloc_live == live && xr_stub_launches == launches, std::string("allocated or launched: ") + buf);
}

Batch make(const char* name, int n_envs, const std::vector<const Reg*>& regs, int force_scratch, int per_region, const std::vector<int32_t>& bounds) {
    return make(name, n_envs, regs, force_scratch, per_region, bounds, [&](Batch& B) {
        Args a;          // before the load: the row size is not known yet, any aligned one is taken as far as the state check
        a.row_bytes = 64;
        call(B, a, std::string(name) + " before the load");
        a.rows_off = 4;
        call(B, a, std::string(name) + " before the load, misaligned rows");
    });
}

// every refusal once, by name, with hostile values, then randomised arguments
void drive(const char* name, Batch& B, Lcg& rng, int random_calls) {
    auto run = [&](Args a, const char* what) { call(B, a, std::string(name) + " " + what); };
    Args a;
    run(a, "valid, defaults");
    a = Args{}; a.out = false; run(a, "null out_dev");
    a = Args{}; a.rows = false; run(a, "null rows_out_dev");
    a = Args{}; a.rows = false; a.out = false; run(a, "null rows_out_dev and out_dev");
    for (int off : {1, 2, 3, 4, 5, 6, 7}) { a = Args{}; a.rows_off = off; run(a, "misaligned rows_out_dev"); }
    a = Args{}; a.rows_off = 8; run(a, "rows_out_dev 8 bytes further");
    for (int64_t extra : {(int64_t)1, (int64_t)4, (int64_t)7, (int64_t)-4, (int64_t)12}) { a = Args{}; a.row_extra = extra; run(a, "row_bytes not a multiple of 8"); }
    a = Args{}; a.row_extra = -8; run(a, "row_bytes 8 below the minimum");
    a = Args{}; a.row_extra = 8; run(a, "row_bytes 8 above the minimum");
    a = Args{}; a.row_bytes = 0; run(a, "row_bytes 0");
    a = Args{}; a.row_bytes = INT32_MAX; run(a, "row_bytes INT32_MAX");
    a = Args{}; a.row_bytes = (int64_t)INT32_MAX + 1; run(a, "row_bytes 2^31");
    a = Args{}; a.row_bytes = INT64_MAX; run(a, "row_bytes INT64_MAX");
    a = Args{}; a.row_bytes = INT64_MAX - 7; run(a, "row_bytes INT64_MAX - 7");
    a = Args{}; a.row_bytes = INT32_MIN; a.row_extra = INT64_MIN; run(a, "row_bytes INT32_MIN");
    a = Args{}; a.row_bytes = INT64_MIN; a.row_extra = INT64_MIN; run(a, "row_bytes INT64_MIN");
    a = Args{}; a.row_bytes = -3; a.row_extra = INT64_MIN; run(a, "row_bytes -3");
    for (int32_t g : {-2, INT32_MIN, INT32_MAX, B.n_groups, B.n_groups + 1}) { a = Args{}; a.group = g; run(a, "group out of range"); }
    a = Args{}; a.group = B.n_groups - 1; run(a, "last group");
    for (int32_t st : {0, -3, INT32_MIN}) { a = Args{}; a.prefix = true; a.prefix_stride = st; run(a, "prefix with a bad stride"); }
    a = Args{}; a.prefix = true; a.prefix_stride = 4; run(a, "prefix with stride 4");
    a = Args{}; a.prefix = true; a.prefix_stride = INT32_MAX; run(a, "prefix with stride INT32_MAX");
    a = Args{}; a.prefix_stride = INT32_MIN; run(a, "no prefix, stride ignored");
    for (int32_t m : {-1, INT32_MIN}) { a = Args{}; a.max_plies = m; run(a, "negative max_plies"); }
    for (int32_t m : {3, INT32_MAX}) { a = Args{}; a.max_plies = m; run(a, "max_plies"); }
    for (int32_t n : {0, -7, INT32_MIN, XR_PEEK_MAX + 1, INT32_MAX}) { a = Args{}; a.n_lines = n; run(a, "n_lines out of range"); }
    a = Args{}; a.n_lines = XR_PEEK_MAX; run(a, "n_lines at the limit");
    for (int32_t k : {B.k_max - 1, 0, -1, INT32_MIN}) { a = Args{}; a.order = true; a.k_cap = k; run(a, "k_cap below k_max with order_out"); }
    for (int32_t k : {B.k_max, INT32_MAX}) { a = Args{}; a.order = true; a.k_cap = k; run(a, "k_cap >= k_max with order_out"); }
    a = Args{}; a.k_cap = INT32_MIN; run(a, "k_cap ignored without order_out");
    a = Args{}; a.ret = false; a.hash = false; run(a, "optional outputs null");
    for (int32_t rb : {INT32_MIN, INT32_MAX, -1}) { a = Args{}; a.region_base = rb; run(a, "any region_base"); }
    for (int i = 0; i < random_calls; i++) {
        Args r;
        r.group = rng.between(-3, B.n_groups + 1);
        r.n_lines = rng.below(4) ? rng.between(1, 9) : (rng.below(2) ? rng.between(-3, 0) : rng.between(XR_PEEK_MAX - 1, XR_PEEK_MAX + 2));
        r.prefix = rng.below(2);
        r.prefix_stride = rng.below(4) ? rng.between(1, 6) : rng.between(-2, 0);
        r.max_plies = rng.below(4) ? rng.between(0, 9) : rng.between(-4, -1);
        r.order = rng.below(2);
        r.k_cap = rng.between(B.k_max - 2, B.k_max + 2);
        r.rows = rng.below(16) != 0; r.out = rng.below(16) != 0; r.ret = rng.below(2); r.hash = rng.below(2);
        r.rows_off = rng.below(6) ? 0 : rng.between(1, 16);
        r.row_extra = rng.below(3) ? 8 * rng.between(0, 4) : rng.between(-24, 24);
        r.region_base = rng.between(-5, 5);
        run(r, "random");
    }
}

}  // namespace

int main() {
    const Reg a(6, 6, 3), b(7, 5, 5);
    Lcg rng{0x9EE4};
    {
        Batch none;          // a null batch, with and without the rest
        Args n;
        n.row_bytes = 64;
        const Expect null_arg{XR_ERR_INVALID, "null argument"};
        call(none, n, "null batch", &null_arg);
        n.out = false;
        call(none, n, "null batch and out_dev", &null_arg);
        n.rows = false; n.rows_off = 3; n.row_bytes = 5;
        call(none, n, "null everything, hostile sizes", &null_arg);
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
        // rows x n_lines beyond 31 bits: 2^19 slots x 4096 lines (one group of the two is small enough)
        const Reg tiny(2, 2, 1);
        const int n = 1 << 19;
        Batch B = make("2^19 slots", n, {&tiny}, 0, 0, {0, n - 1, n});
        const Expect bits{XR_ERR_RANGE, "31 bits"}, unlinked{XR_ERR_STATE, "not linked"};
        Args r;
        r.n_lines = XR_PEEK_MAX;
        call(B, r, "2^19 rows x 4096", &bits);
        r.group = 0;
        call(B, r, "2^19 - 1 rows x 4096", &unlinked);
        r.group = -1; r.n_lines = XR_PEEK_MAX - 1;
        call(B, r, "2^19 rows x 4095", &unlinked);
        xr_batch_destroy(B.h);
        check(xr_stub_alloc_live == 0, "2^19 slots: no device buffer outlives the batch");
    }
    check(xr_stub_launches > 0, "the loads launched their kernels through the stand-in (the counters are live)");
    return finish("PEEK_ARGS");
}
