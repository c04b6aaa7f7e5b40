// tests/hostsan/stub_launch_search.cpp — TEST INFRASTRUCTURE (see hip/hip_runtime.h of this directory): the search launchers that
// xr_device.h declares weak (lookahead, the line launcher, branch, the tree kernels), doing nothing but reporting their arguments to
// xr_stub_search_hook.  Linked by search_trace alone: the *_args programs and libxr_host_asan.so leave these symbols null on purpose, so
// that a valid call answers "not linked" there.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../xroute_env_amd/csrc/xr_device.h"
#include "stub_launch_search.h"

extern "C" {
extern int64_t xr_stub_launches;
void (*xr_stub_search_hook)(const char* launcher, const XrStubArg* args, int n) = nullptr;
}

namespace {
struct Report {
    std::vector<XrStubArg> a;
    Report& i(const char* n, int64_t v) { a.push_back({n, 'i', v, 0, 0.0, nullptr}); return *this; }
    Report& u(const char* n, uint64_t v) { a.push_back({n, 'u', 0, v, 0.0, nullptr}); return *this; }
    Report& f(const char* n, double v) { a.push_back({n, 'f', 0, 0, v, nullptr}); return *this; }
    Report& p(const char* n, const void* v) { a.push_back({n, 'p', 0, 0, 0.0, v}); return *this; }
    // the caller's view of the batch: which slots, and (by its first row) whose rows
    Report& src(const XrBatchDev* d) { return i("src.n_envs", d->n_envs).i("src.env_base", d->env_base).i("src.env_count", d->env_count).p("src.owner", d->owner); }
    // the shadow view: every slot row, the two per-launch rows, and what shadow_view turns off
    Report& shadow(const XrBatchDev* d) {
        i("sh.n_envs", d->n_envs).i("sh.env_base", d->env_base).i("sh.env_count", d->env_count).i("sh.auto_reset", d->auto_reset);
        p("sh.owner", d->owner).p("sh.path", d->path).p("sh.legal", d->legal).p("sh.hash", d->hash).p("sh.reward", d->reward).p("sh.env_steps", d->env_steps);
        p("sh.records", d->records).p("sh.cum", d->cum).p("sh.delta", d->delta).p("sh.nlegal", d->nlegal).p("sh.status", d->status).p("sh.path_len", d->path_len);
        p("sh.sweeps", d->sweeps).p("sh.touched", d->touched).p("sh.env_region", d->env_region).p("sh.env_replay", d->env_replay).p("sh.done", d->done);
        p("sh.total_steps", d->total_steps).p("sh.phase_cycles", d->phase_cycles);
        return p("sh.net_meas", d->net_meas).p("sh.obs_out", d->obs_out).p("sh.obs_out_u8", d->obs_out_u8).p("sh.route_order", d->route_order).p("sh.regions", d->regions);
    }
    Report& variant(const XrRouteVariant& v) { return i("v.lds_dist", v.lds_dist).i("v.zch", v.zch).i("v.lds_bytes", (int64_t)v.lds_bytes).i("v.threads", v.threads); }
    Report& rows(const char* n, const XrSlotRows* r) { return p(n, r->owner); }
    Report& tree(const XrTreeDev* t) {
        p("t.nodes", t->nodes).p("t.rs", t->rs).p("t.prefix", t->prefix).p("t.order", t->order).p("t.ret", t->ret).p("t.E", t->E).p("t.prior", t->prior);
        i("t.node_cap", t->node_cap).i("t.n_par", t->n_par).i("t.k_cap", t->k_cap).i("t.n_sims", t->n_sims).i("t.env_lo", t->env_lo).i("t.e_max", t->e_max);
        p("t.visits_out", t->visits_out).p("t.value_out", t->value_out).p("t.info_out", t->info_out).p("t.best_order_out", t->best_order_out);
        return p("t.best_return_out", t->best_return_out).p("t.paths_out", t->paths_out).p("t.returns_out", t->returns_out);
    }
    Report& keep(const XrTreeKeepDev* k) {
        return p("k.old_nodes", k->old_nodes).p("k.key", k->key).p("k.key_legal", k->key_legal).p("k.played", k->played).p("k.kept_out", k->kept_out).i("k.n_add", k->n_add);
    }
    Report& eval(const XrTreeEvalDev* t) {
        p("t.nodes", t->nodes).p("t.rs", t->rs).p("t.prefix", t->prefix).p("t.ret", t->ret).p("t.leaf", t->leaf).p("t.best_order", t->best_order);
        p("t.legal", t->legal).p("t.nlegal", t->nlegal).p("t.prior", t->prior).p("t.E", t->E);
        return i("t.node_cap", t->node_cap).i("t.n_par", t->n_par).i("t.k_cap", t->k_cap).i("t.e_max", t->e_max).i("t.env_lo", t->env_lo)
            .i("t.legal_words", t->legal_words).i("t.has_prior", t->has_prior);
    }
    hipError_t done(const char* launcher) {
        xr_stub_launches++;
        if (xr_stub_search_hook) xr_stub_search_hook(launcher, a.data(), (int)a.size());
        return hipSuccess;
    }
};

}  // namespace

extern "C" {
hipError_t xr_lookahead_occupancy(XrRouteVariant, int* wg_per_cu) { *wg_per_cu = 1; return hipSuccess; }
hipError_t xr_launch_lookahead_plan(const XrBatchDev* b, int env_lo, int rows, const uint64_t* cand_mask, int32_t* out, double* reward_out, int k_cap, int k_max,
                                    uint32_t* tasks, uint32_t* ctr, uint32_t* next_ctr, hipStream_t) {
    return Report().src(b).i("env_lo", env_lo).i("rows", rows).p("cand_mask", cand_mask).p("out", out).p("reward_out", reward_out).i("k_cap", k_cap).i("k_max", k_max)
        .p("tasks", tasks).p("ctr", ctr).p("next_ctr", next_ctr).done("lookahead_plan");
}
hipError_t xr_launch_lookahead(const XrBatchDev* src, const XrBatchDev* shadow, int env_lo, const uint32_t* tasks, uint32_t* ctr, int32_t* out, double* reward_out,
                               int k_cap, int k_max, XrRouteVariant v, int blocks, hipStream_t) {
    return Report().src(src).shadow(shadow).i("env_lo", env_lo).p("tasks", tasks).p("ctr", ctr).p("out", out).p("reward_out", reward_out).i("k_cap", k_cap)
        .i("k_max", k_max).variant(v).i("blocks", blocks).done("lookahead");
}
// one line per launch, under the kernel's name, in the kernel's argument order
hipError_t xr_launch_line(const XrLineLaunch* l, hipStream_t) {
    const char* const names[] = {"rollout", "rollout_weighted", "peek"};
    static_assert(XR_LINE_POLICY == 0 && XR_LINE_WEIGHTED == 1 && XR_LINE_PEEK == 2, "names[] is indexed by XrLineKind");
    Report r;
    r.src(l->src).shadow(l->shadow).i("env_lo", l->env_lo).i("n_tasks", l->n_tasks).i("per_row", l->per_row);
    if (l->kind == XR_LINE_POLICY) r.i("policy", l->policy);
    if (l->kind != XR_LINE_PEEK) r.u("seed", l->seed);
    r.p("prefix", l->prefix).i("prefix_stride", l->prefix_stride).i("max_plies", l->max_plies).p("ctr", l->ctr).p("next_ctr", l->next_ctr);
    if (l->kind == XR_LINE_PEEK) r.p("rows", l->rows).i("row_bytes", l->row_bytes).i("region_base", l->region_base);
    r.p("out", l->out).p("return_out", l->return_out).p("hash_out", l->hash_out).p("order_out", l->order_out).i("k_cap", l->k_cap);
    if (l->kind == XR_LINE_WEIGHTED) r.p("weights", l->weights).i("weights_k_cap", l->weights_k_cap);
    return r.variant(l->v).i("blocks", l->blocks).done(names[l->kind]);
}
hipError_t xr_launch_weighted_actions(const XrBatchDev* b, const int32_t* weights, int k_cap, int32_t* actions, uint64_t seed, hipStream_t) {
    return Report().src(b).p("weights", weights).i("k_cap", k_cap).p("actions", actions).u("seed", seed).done("weighted_actions");
}
hipError_t xr_launch_branch(const XrSlotRows* env, const XrSlotRows* stg, int env_lo, int rows, const int32_t* parent, int n_max, int path_cap, int legal_words,
                            int chunks, hipStream_t) {
    return Report().rows("env.owner", env).rows("stg.owner", stg).p("stg.done", stg->done).i("env_lo", env_lo).i("rows", rows).p("parent", parent).i("n_max", n_max)
        .i("path_cap", path_cap).i("legal_words", legal_words).i("chunks", chunks).done("branch");
}
hipError_t xr_launch_tree_reset(const XrBatchDev* src, const XrTreeDev* t, int rows, hipStream_t) { return Report().src(src).tree(t).i("rows", rows).done("tree_reset"); }
hipError_t xr_launch_tree_select(const XrBatchDev* src, const XrTreeDev* t, int rows, int wave, hipStream_t) {
    return Report().src(src).tree(t).i("rows", rows).i("wave", wave).done("tree_select");
}
hipError_t xr_launch_tree_backup(const XrBatchDev* src, const XrTreeDev* t, int rows, int wave, int last, hipStream_t) {
    return Report().src(src).tree(t).i("rows", rows).i("wave", wave).i("last", last).done("tree_backup");
}
hipError_t xr_launch_tree_keep_begin(const XrBatchDev* src, const XrTreeDev* t, const XrTreeKeepDev* k, int rows, hipStream_t) {
    return Report().src(src).tree(t).keep(k).i("rows", rows).done("tree_keep_begin");
}
hipError_t xr_launch_tree_eval_open(const XrBatchDev* src, const XrTreeEvalDev* t, const float* root_prior, int rows, hipStream_t) {
    return Report().src(src).eval(t).p("root_prior", root_prior).i("rows", rows).done("tree_eval_open");
}
hipError_t xr_launch_tree_eval_select(const XrTreeEvalDev* t, int32_t* paths_out, int32_t* leaf_out, int rows, hipStream_t) {
    return Report().eval(t).p("paths_out", paths_out).p("leaf_out", leaf_out).i("rows", rows).done("tree_eval_select");
}
hipError_t xr_launch_tree_eval_backup(const XrTreeEvalDev* t, const double* value, const float* leaf_prior, int sims, int32_t* visits_out, double* value_out,
                                      int32_t* info_out, int32_t* best_order_out, double* best_return_out, double* returns_out, int rows, hipStream_t) {
    return Report().eval(t).p("value", value).p("leaf_prior", leaf_prior).i("sims", sims).p("visits_out", visits_out).p("value_out", value_out).p("info_out", info_out)
        .p("best_order_out", best_order_out).p("best_return_out", best_return_out).p("returns_out", returns_out).i("rows", rows).done("tree_eval_backup");
}
}
