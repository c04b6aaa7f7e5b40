// tests/hostsan/args_common.h — TEST INFRASTRUCTURE (see hip/hip_runtime.h of this directory).
//
// What the stand-alone drivers of the search entry points share (tests/hostsan_*/*_args.cpp, search_trace.cpp): the random numbers, the
// failure and call counters, the small region of two-pin nets and a batch made of such regions.  Each program keeps its own arguments,
// expectations and cases.  Included once per program: everything here is file-local.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/xroute_hip.h"

extern "C" int64_t xr_stub_launches;

namespace {

struct Lcg {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)(s >> 33); }
    int below(int n) { return (int)(next() % (uint32_t)n); }
    int between(int lo, int hi) { return lo + below(hi - lo + 1); }
};

int g_failures = 0, g_calls = 0;

[[maybe_unused]] void check(bool ok, const std::string& what) {
    if (ok) return;
    printf("FAILURE: %s\n", what.c_str());
    g_failures++;
}

// a small region: X x Y x 2 nodes, K nets of two access points each
struct Reg {
    int X, Y, Z = 2, K;
    std::vector<int32_t> xs, ys;
    std::vector<uint8_t> dir{0, 1};
    std::vector<uint32_t> nodes;
    Reg(int X_, int Y_, int K_) : X(X_), Y(Y_), K(K_) {
        for (int i = 0; i < X; i++) xs.push_back(1000 + 400 * i);
        for (int i = 0; i < Y; i++) ys.push_back(-500 + 380 * i);
        nodes.assign((size_t)X * Y * Z, XR_TYPE_NORMAL);
        for (int n = 1; n <= K; n++)
            for (int p = 1; p <= 2; p++) nodes[(size_t)((n * 7 + p * 3) % (X * Y)) * Z + (p - 1)] = XR_TYPE_ACCESS | ((uint32_t)n << 3) | ((uint32_t)p << 17);
    }
    xr_region_desc desc() const {
        xr_region_desc d{};
        d.dim_x = X; d.dim_y = Y; d.dim_z = Z;
        d.xs_host = xs.data(); d.ys_host = ys.data(); d.layer_dir_host = dir.data(); d.nodes_host = nodes.data();
        d.n_nets = K;
        return d;
    }
};

struct Expect { int32_t code; const char* msg; };

// the code AND the message of a refusal (which names its entry point), and that the call neither allocated nor launched
[[maybe_unused]] void verdict(const char* fn, int32_t rc, const Expect& want, const std::string& what, int64_t live, int64_t launches) {
    g_calls++;
    const char* msg = xr_last_error();
    char buf[512];
    snprintf(buf, sizeof buf, "%s %s -> rc %d \"%s\", expected %d \"...%s...\"", fn, what.c_str(), rc, msg, want.code, want.msg);
    check(rc == want.code && strstr(msg, fn) && strstr(msg, want.msg), buf);
    check(xr_stub_alloc_live == live && xr_stub_launches == launches, std::string("allocated or launched: ") + buf);
}

struct Batch {
    xr_batch* h = nullptr;
    int n_envs = 0, n_groups = 1, n_max = 0, k_max = 0, legal_words = 0, path_cap = 0;
    int64_t need = 0;          // xr_batch_state_row_bytes
    bool scratch_form = false, loaded = false;
    std::vector<int32_t> bounds;
    int rows(int g) const { return g < 0 || g >= n_groups ? n_envs : bounds[g + 1] - bounds[g]; }
};

// create, before_load(B) (the program's calls on the batch that has no regions yet), load, optional groups
template <class F>
Batch make(const char* name, int n_envs, const std::vector<const Reg*>& regs, int force_scratch, int per_region, const std::vector<int32_t>& bounds,
           F&& before_load) {
    Batch B;
    xr_config c;
    xr_config_default(&c);
    c.n_envs = n_envs; c.force_scratch_field = force_scratch; c.stream_per_region = per_region;
    check(xr_batch_create(&c, &B.h) == XR_OK, std::string(name) + ": create");
    B.n_envs = n_envs; B.bounds = {0, n_envs};
    before_load(B);
    std::vector<xr_region_desc> d;
    for (const Reg* r : regs) d.push_back(r->desc());
    const int32_t rc = xr_batch_load_regions(B.h, d.data(), (int32_t)d.size(), nullptr);
    check(rc == XR_OK, std::string(name) + ": load: " + xr_last_error());
    int32_t s[6] = {0, 0, 0, 0, 0, 0};
    int64_t stride = 0;
    check(xr_batch_sizes(B.h, &s[0], &s[1], &s[2], &s[3], &s[4], &s[5], &stride) == XR_OK, "sizes");
    check(xr_batch_state_row_bytes(B.h, &B.need) == XR_OK && B.need >= 32 && B.need % 8 == 0 && B.need <= 4096, "state row bytes");
    B.n_max = s[2]; B.k_max = s[3]; B.legal_words = s[4]; B.path_cap = s[5];
    B.scratch_form = force_scratch || per_region; B.loaded = true;
    if (!bounds.empty()) {
        check(xr_batch_set_groups(B.h, bounds.data(), (int32_t)bounds.size() - 1) == XR_OK, std::string(name) + ": set_groups: " + xr_last_error());
        B.bounds = bounds; B.n_groups = (int)bounds.size() - 1;
    }
    return B;
}

// the program's last line and exit status: "<TAG>_OK <calls> calls", or "<TAG>_FAILED <failures> of <calls> calls"
[[maybe_unused]] int finish(const char* tag) {
    if (g_failures) printf("%s_FAILED %d of %d calls\n", tag, g_failures, g_calls);
    else printf("%s_OK %d calls\n", tag, g_calls);
    return g_failures ? 1 : 0;
}

}  // namespace
