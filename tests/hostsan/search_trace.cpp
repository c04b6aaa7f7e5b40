// tests/hostsan/search_trace.cpp — TEST INFRASTRUCTURE (see hip/hip_runtime.h of this directory).
//
// Prints, as text, what the host side of the search entry points does on VALID calls: lookahead, rollouts, weighted rollouts, peek, the
// three tree searches, the evaluated tree search's open / leaves / backup, and branch.  The *_args programs of tests/hostsan_* pin the
// refusals and link no search launcher; this program links stub_launch_search.cpp, whose launchers report every argument, and so runs the
// code behind the "not linked" line: pool bring-up, the shadow view, the carvings, the kept pool's half flip, table reuse, the bank
// flips, the eval session's bookkeeping, and every allocation failure on the way.  A line per launch (every scalar; every pointer as
// #<serial of the live allocation that holds it>+<byte offset>, `null`, or `caller`), per hipMalloc, per asynchronous fill / copy, and
// per call its return code and the live allocations (count / bytes).  A structure argument (the views, the variant, the tree descriptors) is written out
// the first time its value is seen in a case, as NAME<k>{...}, and by that name afterwards: the same value, the same name.  The
// allocation-failure walks put a call's events on one line.  No address is printed, so the output is the same on every run.
// tests/test_search_trace.py compares it with search_trace.expected.  Drives the public C ABI only; runs under ASan + UBSan as a
// program of its own (no preload).
#include "args_common.h"
#include "stub_launch_search.h"

#include <algorithm>
#include <functional>
#include <map>

namespace {

// ---- what the hooks see ------------------------------------------------------------------------------------------------------------
struct Alloc { const uint8_t* p; size_t n; int serial; };
std::vector<Alloc> g_live;
int g_serial = 0;            // allocations since the case began (loads included)
bool g_print = false;        // the hooks print (off while a batch is created and loaded)
bool g_brief = false;        // a call's events on one line, launches by name only (the allocation-failure walks)
bool g_again = false;        // ... and of those the allocations only (the call after a refused one: what it still has to allocate)
std::string g_events;        // that line
std::map<std::string, std::string> g_named;          // a structure argument's text -> its name in this case
std::map<std::string, int> g_names;                   // names given so far per structure
int g_fail_in = 0;           // > 0: that many hipMallocs from now, one is refused

void on_alloc(void* p, size_t n, int freed) {
    if (!freed) { g_live.push_back({static_cast<const uint8_t*>(p), n, ++g_serial}); return; }
    g_live.erase(std::remove_if(g_live.begin(), g_live.end(), [&](const Alloc& a) { return a.p == p; }), g_live.end());
}

void on_malloc(size_t bytes) {
    const bool refuse = g_fail_in > 0 && --g_fail_in == 0;
    xr_stub_alloc_limit = refuse ? 0 : -1;          // (this hook runs before the stand-in compares the size with its limit)
    if (!g_print) return;
    if (g_brief) g_events += " malloc " + std::to_string(bytes) + (refuse ? " refused," : ",");
    else printf("  hipMalloc %zu%s\n", bytes, refuse ? " refused" : "");
}

std::string where(const void* ptr) {
    if (!ptr) return "null";
    const uint8_t* p = static_cast<const uint8_t*>(ptr);
    for (const Alloc& a : g_live)
        if (p >= a.p && p < a.p + a.n) return "#" + std::to_string(a.serial) + "+" + std::to_string(p - a.p);
    return "caller";
}

void on_async(const char* what, const void* dst, int kind, size_t bytes) {
    if (!g_print) return;
    const std::string text = std::string(what) + (kind < 0 ? "" : " kind=" + std::to_string(kind)) + " " + where(dst) + " " + std::to_string(bytes);
    if (g_brief) { if (!g_again) g_events += " " + text + ","; }
    else printf("  %s\n", text.c_str());
}

std::string value(const XrStubArg& a) {
    char buf[64];
    if (a.kind == 'i') snprintf(buf, sizeof buf, "%lld", (long long)a.i);
    else if (a.kind == 'u') snprintf(buf, sizeof buf, "0x%llx", (unsigned long long)a.u);
    else if (a.kind == 'f') snprintf(buf, sizeof buf, "%.17g", a.f);
    else return where(a.p);
    return buf;
}

// arguments named "s.field" are the fields of structure s, in a row
void on_launch(const char* launcher, const XrStubArg* a, int n) {
    if (!g_print) return;
    if (g_brief) { if (!g_again) g_events += std::string(" launch ") + launcher + ","; return; }
    printf("  launch %s", launcher);
    for (int i = 0; i < n;) {
        const char* dot = strchr(a[i].name, '.');
        if (!dot) { printf(" %s=%s", a[i].name, value(a[i]).c_str()); i++; continue; }
        const std::string group(a[i].name, dot + 1);
        std::string text;
        for (; i < n && strncmp(a[i].name, group.c_str(), group.size()) == 0; i++) text += std::string(" ") + (a[i].name + group.size()) + "=" + value(a[i]);
        const std::string stem = group.substr(0, group.size() - 1);
        std::string& name = g_named[group + text];
        if (name.empty()) {
            name = stem + std::to_string(++g_names[stem]);
            printf(" %s=%s{%s }", stem.c_str(), name.c_str(), text.c_str());
        } else {
            printf(" %s=%s", stem.c_str(), name.c_str());
        }
    }
    printf("\n");
}

// what a call is made with, on a line of its own before its events (the walks name their call once)
template <class... A>
void say(const char* fmt, A... a) {
    if (!g_brief) printf(fmt, a...);
}

// after each call: its return code (with the message of a refusal) and the live allocations
int32_t said(const char* call, int32_t rc) {
    g_calls++;
    if (g_brief) printf(" %s ", g_events.c_str());          // (a walk: the events and the verdict on one line)
    g_events.clear();
    printf("%s -> rc %d%s%s | live %zu / %lld B\n", call, rc, rc ? ": " : "", rc ? xr_last_error() : "", g_live.size(), (long long)xr_stub_alloc_live);
    return rc;
}

// ---- the caller's buffers: real memory (the leaves call copies line returns into one), contents never looked at ---------------------
std::vector<int32_t> g_out(1 << 14), g_order(1 << 14), g_prefix(1 << 14), g_weights(1 << 14), g_info(1 << 12), g_paths(1 << 14), g_played(64), g_kept(128), g_parent(64);
std::vector<double> g_ret(1 << 12), g_value(1 << 12), g_best_ret(64);
std::vector<uint64_t> g_hash(1 << 12), g_mask(256);
std::vector<float> g_prior(1 << 12);
alignas(16) uint8_t g_rows[1 << 18];

struct Roll { int32_t group = -1, n = 2, policy = XR_ROLLOUT_RANDOM, max_plies = 0; bool prefix = false, order = false, weighted = false; };
struct Peek { int32_t group = -1, n = 2, region_base = 0; bool prefix = true, order = true, ret = true; };
struct Tree { int32_t group = -1, n_waves = 2, n_par = 2, node_cap = 16; double c_init = 1.25, c_base = 19652.0; bool weights = false, keep = false, played = true, extras = true; };
struct Open { int32_t group = -1, n_par = 2, node_cap = 16, max_sims = 4; double c_init = 1.25, c_base = 19652.0; bool prior = false; };

struct Calls {
    Batch& B;
    int32_t lookahead(int32_t group, bool mask = false, bool reward = true) {
        say("lookahead group %d mask %d reward %d\n", group, (int)mask, (int)reward);
        return said("xr_batch_lookahead", xr_batch_lookahead(B.h, group, mask ? g_mask.data() : nullptr, g_out.data(), B.k_max, reward ? g_ret.data() : nullptr, nullptr));
    }
    int32_t rollout(const Roll& a) {
        say("rollout%s group %d n %d policy %d prefix %d order %d max_plies %d\n", a.weighted ? "_weighted" : "", a.group, a.n, a.policy, (int)a.prefix, (int)a.order, a.max_plies);
        const int32_t* prefix = a.prefix ? g_prefix.data() : nullptr;
        int32_t* order = a.order ? g_order.data() : nullptr;
        if (a.weighted)
            return said("xr_batch_rollout_weighted", xr_batch_rollout_weighted(B.h, a.group, a.n, a.policy, 0xABCDEF01ULL, prefix, 3, a.max_plies, g_out.data(), g_ret.data(),
                                                                                g_hash.data(), order, B.k_max + 1, g_weights.data(), B.k_max + 2, nullptr));
        return said("xr_batch_rollout", xr_batch_rollout(B.h, a.group, a.n, a.policy, 0x12345678ULL, prefix, 3, a.max_plies, g_out.data(), g_ret.data(), nullptr, order,
                                                         B.k_max + 1, nullptr));
    }
    int32_t peek(const Peek& a) {
        say("peek group %d n %d prefix %d order %d region_base %d\n", a.group, a.n, (int)a.prefix, (int)a.order, a.region_base);
        return said("xr_batch_peek", xr_batch_peek(B.h, a.group, a.n, a.prefix ? g_prefix.data() : nullptr, 4, 1, g_rows, B.need + 8, a.region_base, g_out.data(),
                                                   a.ret ? g_ret.data() : nullptr, g_hash.data(), a.order ? g_order.data() : nullptr, B.k_max, nullptr));
    }
    int32_t tree(const Tree& a) {
        const char* fn = a.keep ? "xr_batch_tree_search_keep" : a.weights ? "xr_batch_tree_search_weighted" : "xr_batch_tree_search";
        say("%s group %d waves %d par %d node_cap %d c_init %g weights %d played %d extras %d\n", fn + 9, a.group, a.n_waves, a.n_par, a.node_cap, a.c_init, (int)a.weights,
               (int)a.played, (int)a.extras);
        int32_t* best = a.extras ? g_order.data() : nullptr;
        double* best_ret = a.extras ? g_best_ret.data() : nullptr;
        int32_t* paths = a.extras ? g_paths.data() : nullptr;
        double* returns = a.extras ? g_value.data() + 2048 : nullptr;
        const int32_t* w = a.weights ? g_weights.data() : nullptr;
        if (a.keep)
            return said(fn, xr_batch_tree_search_keep(B.h, a.group, a.played ? g_played.data() : nullptr, a.n_waves, a.n_par, 0x5EEDULL, g_prior.data(), a.node_cap, a.c_init,
                                                      a.c_base, g_out.data(), g_value.data(), B.k_max, g_info.data(), best, best_ret, paths, returns, w,
                                                      a.extras ? g_kept.data() : nullptr, nullptr));
        if (a.weights)
            return said(fn, xr_batch_tree_search_weighted(B.h, a.group, a.n_waves, a.n_par, 0x5EEDULL, nullptr, a.node_cap, a.c_init, a.c_base, g_out.data(), g_value.data(),
                                                          B.k_max, g_info.data(), best, best_ret, paths, returns, w, nullptr));
        return said(fn, xr_batch_tree_search(B.h, a.group, a.n_waves, a.n_par, 0x5EEDULL, g_prior.data(), a.node_cap, a.c_init, a.c_base, g_out.data(), g_value.data(), B.k_max,
                                             g_info.data(), best, best_ret, paths, returns, nullptr));
    }
    int32_t open(const Open& a) {
        say("tree_open group %d par %d node_cap %d max_sims %d c_init %g prior %d\n", a.group, a.n_par, a.node_cap, a.max_sims, a.c_init, (int)a.prior);
        return said("xr_batch_tree_open", xr_batch_tree_open(B.h, a.group, a.n_par, a.node_cap, a.c_init, a.c_base, a.max_sims, a.prior ? g_prior.data() : nullptr, B.k_max, nullptr));
    }
    int32_t leaves(int32_t group, bool ret = true) {
        say("tree_leaves group %d return_out %d\n", group, (int)ret);
        return said("xr_batch_tree_leaves", xr_batch_tree_leaves(B.h, group, g_rows, B.need, 0, g_out.data(), ret ? g_ret.data() : nullptr, ret ? g_paths.data() : nullptr,
                                                                 ret ? g_info.data() : nullptr, nullptr));
    }
    int32_t backup(int32_t group, bool extras = true) {
        say("tree_backup group %d extras %d\n", group, (int)extras);
        return said("xr_batch_tree_backup", xr_batch_tree_backup(B.h, group, g_value.data(), extras ? g_prior.data() : nullptr, g_out.data(), g_value.data() + 1024, g_info.data(),
                                                                 extras ? g_order.data() : nullptr, extras ? g_best_ret.data() : nullptr, extras ? g_ret.data() : nullptr, nullptr));
    }
    int32_t branch(int32_t group) {
        say("branch group %d\n", group);
        return said("xr_batch_branch", xr_batch_branch(B.h, group, g_parent.data(), nullptr));
    }
};

Batch begin(const char* name, int n_envs, const std::vector<const Reg*>& regs, const std::vector<int32_t>& bounds, bool header = true) {
    check(g_live.empty(), std::string(name) + ": the last case left allocations");
    g_serial = 0;
    g_named.clear(); g_names.clear();          // (serials start again: a name means its value within a case)
    g_print = false;
    Batch B = make(name, n_envs, regs, 0, 0, bounds, [](Batch&) {});
    if (header) printf("case %s: n_envs %d groups %d k_max %d legal_words %d n_max %d path_cap %d row_bytes %lld | live %zu allocations\n", name, n_envs, B.n_groups, B.k_max, B.legal_words,
           B.n_max, B.path_cap, (long long)B.need, g_live.size());
    g_print = true;
    return B;
}

void end(Batch& B) {
    g_print = false;
    xr_batch_destroy(B.h);
    printf("destroy | live %zu / %lld B\n", g_live.size(), (long long)xr_stub_alloc_live);
    check(g_live.empty() && xr_stub_alloc_live == 0, "a device buffer outlives the batch");
}

// every search call on one batch, in an order that takes every branch of the pools
void drive(Batch& B) {
    Calls c{B};
    const int g1 = 1, g0 = 0;
    // lookahead: the pool is made once per caller, the banks alternate
    c.lookahead(-1); c.lookahead(g1, true, false); c.lookahead(-1);
    // rollouts: the first one adds the claim counters to the pool that lookahead made; twice in a row flips the bank
    Roll r;
    c.rollout(r); c.rollout(r);
    r.prefix = true; r.order = true; r.max_plies = 2; c.rollout(r);
    r.policy = XR_ROLLOUT_STOP; r.order = false; c.rollout(r);
    r = Roll{}; r.weighted = true; r.policy = XR_ROLLOUT_WEIGHTED; c.rollout(r);
    r.prefix = true; r.order = true; c.rollout(r);
    r.policy = XR_ROLLOUT_RANDOM; r.n = 3; c.rollout(r);          // (the weighted entry point with a built-in policy: the plain launch)
    r = Roll{}; r.group = g0; r.n = 4; c.rollout(r);              // a caller without a pool: slots and claim counters at once
    r.weighted = true; r.policy = XR_ROLLOUT_WEIGHTED; c.rollout(r);
    // peek
    Peek p;
    c.peek(p);
    p.order = false; p.ret = false; p.region_base = 7; c.peek(p);
    p = Peek{}; p.prefix = false; p.group = g1; p.n = 3; c.peek(p);
    // tree search: the same knobs twice (no new table, no new allocation), more simulations (a longer table beside the old one), other knobs
    Tree t;
    c.tree(t); c.tree(t);
    t.n_waves = 3; c.tree(t);
    t.n_waves = 1; t.extras = false; c.tree(t);                   // fewer simulations: the longest table serves
    t = Tree{}; t.weights = true; t.n_par = 3; c.tree(t);         // more lanes: the wave memory grows
    t = Tree{}; t.group = g0; c.tree(t);
    t.weights = true; c.tree(t);
    // kept trees: half 0 -> 1 -> 0 with `played` passed on; another node_cap rebuilds; without `played`; with weights; a group caller
    Tree k;
    k.keep = true;
    c.tree(k); c.tree(k); c.tree(k);
    k.node_cap = 24; c.tree(k);
    k.played = false; k.extras = false; c.tree(k);
    k = Tree{}; k.keep = true; k.node_cap = 24; k.n_par = 3; k.weights = true; c.tree(k);          // more lanes: the scratch grows, the trees stay
    k = Tree{}; k.keep = true; k.group = g1; c.tree(k); c.tree(k);
    // evaluated tree search: a session to its last wave and one wave too many; the call order; a second open ends the session
    Open o;
    c.open(o);
    c.leaves(-1); c.backup(-1); c.leaves(-1, false); c.backup(-1, false);
    c.leaves(-1);                                                 // XR_ERR_RANGE: max_sims reached
    c.backup(-1);                                                 // XR_ERR_STATE: no pending leaves
    o.prior = true; o.max_sims = 6; c.open(o);                    // another table length: a new table
    c.leaves(-1); c.leaves(-1);                                   // XR_ERR_STATE: leaves twice
    o.prior = false; c.open(o);                                   // ends the session with its leaves pending; same knobs: the table is reused
    c.backup(-1);                                                 // XR_ERR_STATE: the new session has no leaves yet
    c.leaves(-1); c.backup(-1);
    o = Open{}; o.group = g1; o.n_par = 3; o.node_cap = 32; c.open(o);
    c.leaves(g1); c.backup(g1);
    c.leaves(0);                                      // XR_ERR_STATE: no session of that caller
    // branch: the staging rows are made once per caller
    c.branch(-1); c.branch(-1); c.branch(g1);
}

// Every allocation of an entry point refused in turn, on a fresh batch each time: the documented XR_ERR_NOMEM, the same call again
// succeeding, and nothing left after the batch is destroyed.  `setup` runs first, unrefused (the pools a call builds on)
void walk_nomem(const char* name, const std::vector<const Reg*>& regs, const std::function<void(Calls&)>& setup, const std::function<int32_t(Calls&)>& call) {
    for (int n = 1; n < 32; n++) {
        Batch B = begin(name, 5, regs, {0, 2, 5}, n == 1);          // (the same batch every time: its line once)
        Calls c{B};
        g_brief = true;
        g_print = false;
        setup(c);
        g_print = true;
        printf("refusing hipMalloc %d:", n);
        g_fail_in = n;
        const int32_t rc = call(c);
        const bool refused = g_fail_in == 0;
        g_fail_in = 0;
        xr_stub_alloc_limit = -1;
        if (refused) {
            check(rc == XR_ERR_NOMEM, std::string(name) + ": a refused hipMalloc must answer XR_ERR_NOMEM");
            printf("the same call again:");
            g_again = true;
            check(call(c) == XR_OK, std::string(name) + ": the call after a refused one must succeed");
        } else {
            check(rc == XR_OK, std::string(name) + ": an unrefused call must succeed");
            printf("(the call makes %d allocations)\n", n - 1);
        }
        end(B);
        g_brief = g_again = false;
        if (!refused) return;
    }
    check(false, std::string(name) + ": more than 31 allocations in one call");
}

}  // namespace

int main() {
    xr_stub_alloc_hook = on_alloc;
    xr_stub_malloc_hook = on_malloc;
    xr_stub_async_hook = on_async;
    xr_stub_search_hook = on_launch;
    const Reg a(6, 5, 3), b(7, 4, 2), big(9, 8, 70), bare(4, 4, 0);
    {
        Batch B = begin("two regions, three callers", 5, {&a, &b}, {0, 2, 5});
        drive(B);
        end(B);
    }
    {
        // what the number of legal words enters: the shadow slots, the packed rows, the kept pool's keys, the session's snapshot, the staging rows
        Batch B = begin("a region of 70 nets: two legal words, one caller", 3, {&a, &b, &big}, {});
        Calls c{B};
        c.lookahead(-1);
        Roll r; r.order = true; c.rollout(r);
        c.peek(Peek{});
        c.tree(Tree{});
        Tree k; k.keep = true; c.tree(k); c.tree(k);
        c.open(Open{}); c.leaves(-1); c.backup(-1);
        c.branch(-1);
        end(B);
    }
    {
        Batch B = begin("no nets", 2, {&bare}, {});
        Calls c{B};
        c.lookahead(-1); c.lookahead(-1);          // k_max < 1: the fill of the planning pass is the whole answer
        end(B);
    }
    {
        // a kept search whose table is refused flips no half: the call after it reads the half the last successful call wrote
        Batch B = begin("kept halves after a refused table", 5, {&a, &b}, {});
        Calls c{B};
        Tree k; k.keep = true; c.tree(k);
        k.c_init = 2.5;                            // other knobs: the only allocation of the call is its table
        g_fail_in = 1;
        check(c.tree(k) == XR_ERR_NOMEM && g_fail_in == 0, "the table of the second kept call is refused");
        xr_stub_alloc_limit = -1;
        c.tree(k);
        end(B);
    }
    const std::vector<const Reg*> regs{&a, &b};
    auto none = [](Calls&) {};
    walk_nomem("lookahead", regs, none, [](Calls& c) { return c.lookahead(-1); });
    walk_nomem("rollout", regs, none, [](Calls& c) { return c.rollout(Roll{}); });
    walk_nomem("rollout after lookahead", regs, [](Calls& c) { c.lookahead(1); }, [](Calls& c) { Roll r; r.group = 1; return c.rollout(r); });
    walk_nomem("rollout_weighted", regs, none, [](Calls& c) { Roll r; r.weighted = true; r.policy = XR_ROLLOUT_WEIGHTED; return c.rollout(r); });
    walk_nomem("peek", regs, none, [](Calls& c) { return c.peek(Peek{}); });
    walk_nomem("tree_search", regs, none, [](Calls& c) { return c.tree(Tree{}); });
    walk_nomem("tree_search, a longer table", regs, [](Calls& c) { c.tree(Tree{}); }, [](Calls& c) { Tree t; t.n_waves = 4; t.n_par = 3; return c.tree(t); });
    walk_nomem("tree_search_keep", regs, none, [](Calls& c) { Tree t; t.keep = true; return c.tree(t); });
    walk_nomem("tree_search_keep, another shape", regs, [](Calls& c) { Tree t; t.keep = true; c.tree(t); },
               [](Calls& c) { Tree t; t.keep = true; t.node_cap = 64; t.n_par = 4; return c.tree(t); });
    walk_nomem("tree_open", regs, none, [](Calls& c) { return c.open(Open{}); });
    walk_nomem("tree_open, a larger session", regs, [](Calls& c) { c.open(Open{}); c.leaves(-1); },
               [](Calls& c) { Open o; o.node_cap = 64; o.max_sims = 8; return c.open(o); });
    walk_nomem("tree_leaves", regs, [](Calls& c) { c.open(Open{}); }, [](Calls& c) { return c.leaves(-1); });
    walk_nomem("branch", regs, none, [](Calls& c) { return c.branch(1); });
    check(xr_stub_launches > 0, "the calls launched through the stand-in");
    if (g_failures) printf("SEARCH_TRACE_FAILED %d of %d calls\n", g_failures, g_calls);
    else printf("SEARCH_TRACE_OK\n");
    return g_failures ? 1 : 0;
}
