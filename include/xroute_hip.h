/*
 * xroute_hip.h — C ABI of libxroute_hip.so: the MI355X (gfx950) in-process replacement for the
 * reference's env hot path  Game.reset()/Game.step()  (simulator round trip + build_3Dgrid + metric
 * deltas + reward).
 *
 * The reference has no FFI for this path: the seam is the Python `Game` object and the protobuf
 * `Message` behind it.  Every entry point below names the reference interface it
 * replaces.  All paths are relative to the reference repository root.
 *
 * Conventions
 *   - plain C types only; every function returns an int32_t status (XR_OK == 0, negative = error);
 *     xr_last_error() returns a thread-local message for the last failing call on this thread;
 *   - no exception crosses the ABI;
 *   - `stream` arguments are a hipStream_t passed as void* (pass torch's current stream);
 *     functions only enqueue work on it and never synchronise unless documented ("sync");
 *   - pointers named *_dev are device pointers on the batch's device, *_host are host pointers;
 *     the caller owns every buffer it passes; the library owns batch state until xr_batch_destroy;
 *   - calls on one batch must be serialised by the caller; one batch is bound to one HIP device;
 *   - net ids are 1-based at this boundary exactly as in the reference's env API
 *     (baseline/baseline_utils.py:20,26,33 shift the wire's 0-based ids by +1; Game.step sends
 *     action-1, :410).
 *
 * Node records (uint32), flat node order f = (x*Y + y)*Z + z  (the memory order of the reference
 * observation: baseline/build_3Dgrid.py:97-103 reshapes a zeros([X,Y,Z]) tensor without permuting):
 *   bits  1:0  type  0 BLOCKAGE 1 NORMAL 2 ACCESS     (baseline/openroad_api/proto/net_ordering.proto:5-9)
 *   bit   2    is_used                                (net_ordering.proto:24)
 *   bits 16:3  net+1 (0 = none)                       (net_ordering.proto:25)
 *   bits 30:17 pin+1 (0 = none)                       (net_ordering.proto:26)
 */
#ifndef XROUTE_HIP_H
#define XROUTE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XR_ABI_VERSION 9

/* status codes */
#define XR_OK            0
#define XR_ERR_INVALID  (-1)   /* bad argument */
#define XR_ERR_NOMEM    (-2)   /* host or device allocation failed */
#define XR_ERR_HIP      (-3)   /* a HIP runtime call failed (message has the HIP error string) */
#define XR_ERR_STATE    (-4)   /* call order violated (e.g. step before load_regions) */
#define XR_ERR_RANGE    (-5)   /* size/limit exceeded (dims, net count, LDS capacity ...) */
#define XR_ERR_PARSE    (-6)   /* malformed protobuf bytes */

/* node record fields */
#define XR_TYPE_BLOCKAGE 0u
#define XR_TYPE_NORMAL   1u
#define XR_TYPE_ACCESS   2u
#define XR_REC_TYPE(r)   ((r) & 3u)
#define XR_REC_USED(r)   (((r) >> 2) & 1u)
#define XR_REC_NET1(r)   (((r) >> 3) & 0x3FFFu)    /* net + 1, 0 = none */
#define XR_REC_PIN1(r)   (((r) >> 17) & 0x3FFFu)   /* pin + 1, 0 = none */
#define XR_MAX_NETS      16382
#define XR_MAX_LAYERS    32
/* Track coordinates (xr_region_desc.xs_host / ys_host) lie in [-2^30, 2^30], both ends included, and the tracks of one axis of a
 * region span less than XR_MAX_TRACK_SPAN DBU (last - first; XR_ERR_RANGE otherwise): the routers keep coordinates relative to the
 * first track, x4, in 32-bit words and add two spans in the search heuristic.  The spec loses nothing: a distance of XR_DIST_CAP =
 * 0x07F00000 (< 2^27) or more does not exist, so an edge that long is never crossed.  Costs: via_cost, guide_cost and
 * drc_cost * drc_unit << (maze_end_iter - 1) are each below 2^22 (xr_batch_create) */
#define XR_MAX_TRACK_SPAN (1ll << 28)

/* owner value of nodes occupied by something that is not a net of this region
 * (blockages, pre-routed wires: is_used NORMAL nodes in the initial Request) */
#define XR_OWNER_FOREIGN 0x7FFF

/* per-env status bits (XR_FETCH_STATUS) */
#define XR_ENV_OK            0
#define XR_ENV_BAD_ACTION    1   /* action not in the legal set: step was a no-op (the reference does
                                    not check this client-side, baseline/baseline_utils.py:409-412) */
#define XR_ENV_UNREACHABLE   2   /* at least one pin could not be reached */
#define XR_ENV_PATH_TRUNC    4   /* path longer than path_cap: path list truncated, metrics exact */
#define XR_ENV_WAS_RESET     8   /* auto_reset: this step re-initialised the env instead of routing */
#define XR_ENV_ROUTER_ABORT 16   /* the router gave up on this net: a search exceeded its round cap (1024 + N relaxation rounds, far
                                    beyond anything a legal region needs; xr_config.debug_round_cap forces it).  The pins not
                                    connected yet are charged as unreachable; the env stays consistent and the device never
                                    spins on a pathological region */

typedef struct xr_batch xr_batch;

/* Router / env parameters.  The simulator knobs mirror the reference's TCL
 * (ispd/ispd18_test1/run-net-ordering-training.tcl:3 `-drc_cost 8`), the reward weights its
 * trainers (baseline/DQN/train_DQN.py:98-99, baseline/PPO/train_PPO.py:101-102), max_route_count
 * its control plane (examples/launch_training.py:28). */
#define XR_ROUTER_SWEEP 1
#define XR_ROUTER_DIAL  2
#define XR_ROUTER_DIAL_R2 3   /* round 2's LDS form of the frontier router (four waves per search, mask scans): kept for A/B runs */
#define XR_OBS_FUSED 1
#define XR_OBS_SPLIT 2
#define XR_OBS_QUEUE 3
typedef struct xr_config {
    int32_t struct_size;      /* = sizeof(xr_config); checked */
    int32_t device;           /* HIP device ordinal */
    int32_t n_envs;           /* B: env slots in this batch */
    int32_t via_cost;         /* XR-Maze v1: cost of one via edge, DBU-equivalent (default 800) */
    int32_t drc_cost;         /* default 8 */
    int32_t drc_unit;         /* DBU per drc_cost unit (default 400): entering a node held by
                                 another net costs drc_cost*drc_unit and counts one violation */
    int32_t max_route_count;  /* replays of one region before rotating to the next (default 10) */
    int32_t auto_reset;       /* 1: xr_batch_step re-initialises envs that were done (vector env) */
    int32_t path_cap;         /* max recorded path nodes per env-step (0 = min(N, 4096)) */
    int32_t block_threads;    /* route kernel workgroup size, 0 = default */
    int32_t force_scratch_field; /* 1: keep the distance field in HBM scratch even when it would fit LDS (the
                                    large-region code path; for tests and A/B measurements) */
    int32_t obs_mode;         /* xr_batch_step_observe: 0 = default (XR_OBS_QUEUE where it applies, the fastest as measured,
                                 else XR_OBS_FUSED), XR_OBS_FUSED = one launch of one workgroup per env, XR_OBS_SPLIT = route
                                 kernel + concurrent net-plane writer, XR_OBS_QUEUE = planning kernel + one persistent launch */
    double  w_violation;      /* 500  */
    double  w_via;            /* 4    */
    double  w_wirelength;     /* 0.5  */
    int32_t obs_writer_blocks; /* XR_OBS_SPLIT: workgroups of the net-plane writer; XR_OBS_QUEUE: workgroups of the
                                  persistent launch (0 = default: 512 / as many as are resident on the chip) */
    int32_t router;           /* XR-Maze v1 relaxation scheme (same results, bit for bit): 0 = auto (XR_ROUTER_DIAL wherever it applies;
                                 only the full-rewrite queue launch of a batch of >= 4096 slots takes XR_ROUTER_SWEEP, measured
                                 1-2 % faster there), XR_ROUTER_SWEEP = line-segment sweeps over dirty-line
                                 worklists (round 1), XR_ROUTER_DIAL = bucketed frontier expansion (Dial's algorithm with A* keys; regions that fit
                                 LDS take round 3's form — mask rounds, quads of lanes per chain, predecessor directions in the field word — whenever one
                                 edge with its penalties stays below 2^20; larger regions the HBM-scratch form), XR_ROUTER_DIAL_R2 = round 2's LDS form of it */
    int32_t dial_mult;        /* XR_ROUTER_DIAL: bucket width in units of the region's smallest edge length (0 = default 8) */
    int32_t guide_cost;       /* XR-Maze v2 (all three neutral by default = XR-Maze v1): entering a node outside the net's guide costs this
                                 much extra, DBU-equivalent (the role of `-follow_guide 1`, run-net-ordering-training.tcl:3); the guide of
                                 a net = bounding box of all its access points in track indices, inflated by guide_margin, every layer */
    int32_t guide_margin;
    int32_t maze_end_iter;    /* >= 1 (`-maze_end_iter 3 -ripup_mode 1` of the same line): attempt t routes the net with the penalty
                                 drc_cost*drc_unit << t; an attempt whose path uses a node held by another net is ripped up unless it is
                                 the last one.  Frontier router only (XR_ROUTER_SWEEP: XR_ERR_RANGE) */
    int32_t stream_per_region; /* 1: "one region per stream" (north_star's first partition): xr_batch_step / _step_observe (fused
                                  form) / _step_compact launch ONE single-workgroup kernel per env slot, round-robin over a pool of
                                  internal HIP streams, joined to the caller's stream by events.  For batches of <= 64 slots only
                                  (XR_ERR_RANGE above); measured against the default one-launch form in DESIGN.md */
    int32_t obs_helper_blocks; /* XR_OBS_QUEUE: LDS-free helper-writer workgroups launched beside the persistent step kernel on an
                                  internal stream, draining the same unit queue (0 = none, the default: measured no faster) */
    int32_t obs_split_permille; /* XR_OBS_SPLIT: per mille of every env's net planes (its highest-ranked nets) that the
                                   writer kernel streams; the step kernel writes the rest after routing (0 = 1000 = all).
                                   XR_OBS_QUEUE: units a workgroup writes after each route task, per mille of the average
                                   number of units per env (0 = 750) */
    int32_t launch_order;     /* route-only launches (xr_batch_step, xr_batch_step_compact, fused xr_batch_step_observe): order in
                                 which the env slots are handed to workgroups.  0 = default: longest predicted route first when
                                 the batch has more slots than the chip holds workgroups (a ~10 us ordering kernel ahead of the
                                 launch; the prediction is the chosen net's bounding box and pin count), slot order otherwise;
                                 1 = slot order always; 2 = longest first always.  The queue form of xr_batch_step_observe hands its
                                 ROUTE TASKS out the same way: 0 = longest first for batches of at most 2 routes per resident workgroup (4
                                 with planes that are not 16-byte aligned), slot order above that; 1 / 2 as above.  Results do not depend on it.  (Takes the
                                 struct's former tail padding: sizeof(xr_config) is unchanged.) */
    int32_t debug_round_cap;  /* 0 = default.  > 0: relaxation rounds one search of the router may take before it aborts with
                                 XR_ENV_ROUTER_ABORT (tests force the abort path with 1) */
    int32_t window;           /* regions whose distance field does not fit LDS (BASELINE config 5), > 0: the router first runs inside an LDS window
                                 of the region centred on the net (the largest square window of at most this many tracks that fits LDS: 52 at 12
                                 layers) and accepts the result only with an exactness certificate — no shortest path to anything the step looks
                                 at leaves the window — else the HBM-scratch form routes the net.  0 (default) / < 0: off — built and bit-exact,
                                 but measured no faster than the HBM-scratch form alone on config 5.  Results never depend on
                                 it.  (ABI 6; was reserved0 = 0.) */
} xr_config;

/* One region = one simulator Request (net_ordering.proto:29-45) in dense form; host pointers. */
typedef struct xr_region_desc {
    int32_t dim_x, dim_y, dim_z;
    const int32_t*  xs_host;        /* [dim_x] track coordinates (Node.point_x), strictly increasing */
    const int32_t*  ys_host;        /* [dim_y] */
    const uint8_t*  layer_dir_host; /* [dim_z] 0 = horizontal (x moves), 1 = vertical (y moves) */
    const uint32_t* nodes_host;     /* [X*Y*Z] packed records */
    int32_t n_nets;                 /* nets 1..n_nets may appear in records */
    int32_t metrics0[3];            /* cumulative (violation, wirelength, via) of the initial Request
                                       (Request.reward_*, net_ordering.proto:36-38) */
} xr_region_desc;

/* what xr_batch_fetch copies (device -> caller's buffer: a DEVICE buffer or PINNED host memory; async on `stream`) */
#define XR_FETCH_CUM       0   /* int32 [B][3]  cumulative (violation, wirelength, via)  = data[2] */
#define XR_FETCH_DELTA     1   /* int32 [B][3]  last step's deltas  (Game.step :426-433) */
#define XR_FETCH_REWARD    2   /* double[B]     -(wv*dvio + wvia*dvia + wwl*dwl)  (train_DQN.py:98-99) */
#define XR_FETCH_DONE      3   /* uint8 [B]     len(netSet)==0  (Game.step :435-436) */
#define XR_FETCH_NLEGAL    4   /* int32 [B]     len(netSet) */
#define XR_FETCH_STATUS    5   /* int32 [B]     XR_ENV_* bits of the last step */
#define XR_FETCH_LEGAL     6   /* uint64[B][legal_words] bit n-1 set <=> net n in netSet */
#define XR_FETCH_PATH_LEN  7   /* int32 [B]     nodes claimed by the last step (untruncated count) */
#define XR_FETCH_PATH      8   /* int32 [B][path_cap] flat node ids in back-trace order */
#define XR_FETCH_OWNER     9   /* int16 [B][n_max] per-node owner (0 free, net id, XR_OWNER_FOREIGN) */
#define XR_FETCH_HASH     10   /* uint64[B]     FNV-1a chain over every (path, deltas) since reset_all */
#define XR_FETCH_REGION   11   /* int32 [B]     region index the env currently plays */
#define XR_FETCH_STEPS    12   /* int64 [1]     env-steps (real routes, not resets) since create */
#define XR_FETCH_SWEEPS   13   /* int32 [B]     relaxation sweeps used by the last step */
#define XR_FETCH_RECORD   15   /* xr_step_record[B]  everything a caller needs after a step or a reset, one 48-byte
                                                 record per env (written by the kernels themselves: one copy, one sync) */
#define XR_FETCH_TOUCHED  16   /* int32 [B]     nodes whose field word the last route created (HBM-scratch form of the frontier
                                                 router: the work it really did; 0 for the other forms) */
#define XR_FETCH_UNITS    17   /* uint32[1]     net-plane units (7 planes of one net of one env) the last xr_batch_step_observe* planned */
#define XR_FETCH_ROUTE_ORDER 18 /* int32[B]     env slots in the order the last longest-first route-only launch handed them out (xr_config.launch_order) */
#define XR_FETCH_REPLAY   19   /* int32 [B]     replays of the current region so far (region rotation, examples/launch_training.py:28-46) */
#define XR_FETCH_ENV_STEPS 20  /* int64 [B]     real steps of every env slot since create */
#define XR_FETCH_PHASES   14   /* int64 [B][8]  slot 7: shader-clock cycles of the env's last route (frontier router; what the measured launch order
                                                 is built from — bench.py's launch utilisation = mean / max over a launch); slots 0..6: route-kernel
                                                 phase cycle counts, zero unless the library was built with -DXR_PHASE_TIMING (which also owns slot 7) */

/* Per-env result of the last xr_batch_step* / xr_batch_reset: what Game.step returns besides the observation
 * (baseline/baseline_utils.py:426-439) plus what Game.reset records (:472-473), packed for one transfer — also the
 * record that the multi-GPU gather exchanges (one all_gather of B x 48 bytes per step). */
typedef struct xr_step_record {
    double   reward;       /* -(500 dvio + 4 dvia + 0.5 dwl), train_DQN.py:98-99 */
    int32_t  delta[3];     /* violation, wirelength, via of the last step */
    int32_t  cum[3];       /* cumulative metrics (data[2]) */
    int32_t  nlegal;       /* len(netSet) */
    int32_t  env_steps;    /* real steps of this env slot since create (low 32 bits) */
    int32_t  path_len;
    uint8_t  done;
    uint8_t  pad;
    uint16_t status;       /* XR_ENV_* bits */
} xr_step_record;

int32_t     xr_abi_version(void);
const char* xr_last_error(void);
void        xr_config_default(xr_config* cfg);
int32_t     xr_device_count(int32_t* n);

/* ---- batch life cycle ------------------------------------------------------------------- */
int32_t xr_batch_create(const xr_config* cfg, xr_batch** out);
int32_t xr_batch_destroy(xr_batch* b);

/* Replaces: receiving the initial Request of each region dump (examples/launch_training.py:57-64
 * relaunching the simulator on a `workerx*_y*` dir; baseline/baseline_utils.py:459-466).
 * Uploads the regions and runs the ingest kernel (records -> compact node_net/owner0 state + per-net
 * access-point lists).  Env e initially plays region e % n_regions.  Synchronises `stream`. */
int32_t xr_batch_load_regions(xr_batch* b, const xr_region_desc* regions_host, int32_t n_regions,
                              void* stream);

/* env -> region assignment (host array of n_envs region indices); takes effect at the next reset */
int32_t xr_batch_assign(xr_batch* b, const int32_t* env_region_host);

/* Sizes the caller needs for its buffers. */
int32_t xr_batch_sizes(const xr_batch* b, int32_t* n_envs, int32_t* n_regions, int32_t* n_max,
                       int32_t* k_max, int32_t* legal_words, int32_t* path_cap, int64_t* obs_env_stride);

/* Replaces Game.reset (baseline/baseline_utils.py:441-481) + the control plane's region rotation
 * (examples/launch_training.py:33-54).  mask_dev: uint8[B] (nonzero = reset this env) or NULL = all.
 * rotate != 0 applies the 10-replays-then-next-region policy, 0 replays the assigned region. */
int32_t xr_batch_reset(xr_batch* b, const uint8_t* mask_dev, int32_t rotate, void* stream);

/* Replaces Game.step's simulator round trip (baseline/baseline_utils.py:409-419: send net_index =
 * action-1, receive the next Request) and its metric bookkeeping (:426-438): routes net
 * actions_dev[e] (1-based) in env e with the XR-Maze v1 router, claims the path nodes, accumulates
 * wirelength/via/violation, updates netSet/done/reward. */
int32_t xr_batch_step(xr_batch* b, const int32_t* actions_dev, void* stream);

/* Game.step with its observation (baseline/baseline_utils.py:409-423: route, then build_3Dgrid on the new state),
 * out_dev / env_stride as in xr_batch_observation, for envs [0, n_envs).  Three forms, same bytes:
 *   XR_OBS_FUSED  one launch: every workgroup routes its env, then streams that env's observation.
 *   XR_OBS_SPLIT  the 7K net planes of an env do not depend on the routing result (they are functions of the
 *                 region's static node array and of which nets remain, which follows from the state before the
 *                 step), so a planning kernel derives every env's post-step net set, a balanced, address-ordered
 *                 writer kernel streams all net planes on an internal stream, and the route kernel — running
 *                 concurrently on the caller's stream — writes planes 0..1.  The caller's stream is joined with
 *                 the internal one before the call returns control of the stream (event wait, no host sync).
 *                 Needs a 16-byte aligned out_dev and env_stride % 4 == 0 (regions whose N is not a multiple of 4 take
 *                 a writer that resolves plane boundaries per float); otherwise the call runs XR_OBS_FUSED.
 *   XR_OBS_QUEUE  (default) the same planning kernel, then ONE persistent launch on the caller's stream whose workgroups
 *                 drain two task queues: envs to route (+ their planes 0..1) and net-plane units to write.  Units do not
 *                 depend on routing, so they keep HBM busy while other workgroups route and the launch ends in a
 *                 fine-grained pure-write drain instead of a tail of whole envs.  Same requirements as XR_OBS_SPLIT. */
int32_t xr_batch_step_observe(xr_batch* b, const int32_t* actions_dev, float* out_dev, int64_t env_stride,
                              void* stream);

/* In-place form of xr_batch_step_observe for a caller that keeps ONE observation buffer for the batch (the vector env): the
 * planes of a net are static (baseline/build_3Dgrid.py:106-142) and the channel order is "nets ascending" (:177-179), so removing
 * the routed net shifts only the nets ABOVE it down by one 7-plane slot — the nets below keep their slot and their bytes.
 * When out_dev / env_stride are the buffer that received this batch's previous full observation (the last xr_batch_observation
 * over all slots, xr_batch_step_observe or xr_batch_step_observe_inplace, with no other state-changing call in between) and
 * the caller has not written to it, only planes 0..1 and the planes of the remaining nets above the routed one are written
 * (a slot that re-initialises writes everything, a rejected action planes 0..1 only): the buffer ends up byte-identical to
 * what xr_batch_step_observe writes, with about half the HBM traffic under a uniform net choice.  Any other buffer: a full
 * write, exactly xr_batch_step_observe.  xr_batch_observe_timing reports mode | 16 when the in-place path ran (and mode | 32
 * when the auto router ran the line-segment sweeps in the queue launch: full rewrite of a batch of >= 4096 slots). */
int32_t xr_batch_step_observe_inplace(xr_batch* b, const int32_t* actions_dev, float* out_dev, int64_t env_stride,
                                      void* stream);

/* Compact-consumer mode.  The reference consumer re-encodes every net's 7 planes at every step (baseline/DQN/DQN.py:138-155),
 * but those planes are functions of the region's static access points only (baseline/build_3Dgrid.py:106-142): a consumer
 * that caches per-(region, net) results (xroute_env_amd.agents.NetVectorCache) needs, per step, only the two planes that
 * change — plane 0 (obstacles) and plane 1 (net order).
 *   xr_batch_step_compact  = xr_batch_step + planes 0..1 of every env at head_out_dev + e*head_stride (floats; 16-byte
 *                            aligned buffer, head_stride % 4 == 0, head_stride >= 2*n_max): 8·N bytes per env-step instead
 *                            of 4·N·(2+7K).
 *   xr_batch_net_planes    = the 7 planes [7, Z, Y, X] of n_pairs (region index, 1-based net id) pairs, pair i at
 *                            out_dev + i*pair_stride (floats, pair_stride >= 7*n_max) — byte-identical to planes 2+7i..8+7i
 *                            of xr_batch_observation for an env playing that region with that net at rank i.  A net id that
 *                            names no net of the region (<= 0, > n_nets) gives seven planes of zeros.  A pair whose region index
 *                            is outside the table (< 0, >= n_regions) is passed over: its row of out_dev is NOT written, the
 *                            other pairs are.  Of a pair's row only the first 7*N floats (N = nodes of ITS region) are written. */
int32_t xr_batch_step_compact(xr_batch* b, const int32_t* actions_dev, float* head_out_dev, int64_t head_stride,
                              void* stream);
int32_t xr_batch_net_planes(xr_batch* b, const int32_t* pair_region_dev, const int32_t* pair_net_dev, int32_t n_pairs,
                            float* out_dev, int64_t pair_stride, void* stream);

/* Compact state for a CENTRAL learner (ABI 7; SURVEY.md §8e, BASELINE config 4).  The reference's caller loop evaluates its policy on the
 * observation of the env it just stepped (baseline/PPO/train_PPO.py:96-99: `action = ppo_agent.select_action(state); state, ... = game.step(action)`).
 * When ONE learner process evaluates the policy for env slots that live on other GPUs, what has to travel per env-step is not the two fp32
 * planes that change (8·N bytes) but what they are functions of: plane 0 (obstacle: blockage or used, baseline/build_3Dgrid.py:19-36,94-103) is
 * one bit per node, plane 1 (the remaining nets' ids ascending at flat positions 0..K-1, :144-161) is the legal-net bitmask.
 *   xr_batch_state_row_bytes  bytes of one packed row of THIS batch: 16 + 8·(legal_words + ceil(n_max / 64)); ranks agree on the maximum.
 *   xr_batch_pack_state       one row per env slot at rows_dev + e*row_bytes (8-byte aligned, row_bytes % 8 == 0):
 *                               int32 region + region_base | int32 nlegal | int32 legal_words | int32 occ_words |
 *                               uint64 legal[legal_words] | uint64 occ[occ_words]  (bit f%64 of word f/64 = node f, flat observation order)
 *                             region_base: what turns this batch's local region index into an index of the learner's region table.
 *                             occ_words is ceil(n_max / 64) for every slot of the batch; bits at and beyond the N nodes of the slot's own
 *                             region are zero, whatever the owner row holds behind N.  row_bytes may exceed xr_batch_state_row_bytes
 *                             (ranks agree on the maximum): the bytes of a row beyond 16 + 8·(legal_words + occ_words) are NEVER
 *                             written — they keep what the caller put there, and xr_batch_expand_state never reads them.
 *   xr_batch_expand_state     (learner side; `b` supplies the region table: it must hold every region the rows name) n_rows rows -> the
 *                             fp32 head rows xr_batch_step_compact writes for those envs, byte for byte (planes 0..1 at
 *                             head_out_dev + i*head_stride, each env in its own region's layout), plus nlegal / region of every row as
 *                             int32 arrays for xr_agent_actor.  A row that does not parse (region outside the table, sizes that do not
 *                             fit, nlegal != popcount(legal), a legal bit beyond the region's nets) is left unwritten and flagged
 *                             nlegal = region = -1. */
int32_t xr_batch_state_row_bytes(const xr_batch* b, int64_t* row_bytes);
/* The client half of Game.step WITHOUT the route (ABI 9; BASELINE config 2: "grid-build + reward only"): a new state of every env slot, as an
 * external simulator's `Request` carries it, becomes the batch's state — replaces baseline/baseline_utils.py:420-438 for a batch (`data =
 * handle_messange(..)`; the metric deltas `*_cur_step - *_last_step`, :426-433; `done = len(netSet) == 0`, :435-436) with the trainers' reward
 * (baseline/DQN/train_DQN.py:98-99, double) computed in the same kernel.  Follow it with xr_batch_observation for the fp32 grid (build_3Dgrid, :423).
 *   owner_dev   int16 [n_envs][n_max]        occupancy of every node in flat order: 0 free, the 1-based net id holding it, XR_OWNER_FOREIGN
 *                                            (16-byte aligned rows: n_max is a multiple of 8)
 *   legal_dev   uint64 [n_envs][legal_words] bit n-1 = net n is still to route (`Request.nets`, +1); bits beyond the region's nets are dropped
 *   cum_dev     int32 [n_envs][3]            cumulative violation / wirelength / via (`reward_violation`, `reward_wire_length`, `reward_via`)
 * Afterwards XR_FETCH_RECORD / _DELTA / _REWARD / _DONE / _NLEGAL describe the step; env_steps advanced by one; the hash chain (routed paths) is
 * untouched.  Enqueues one kernel, never synchronises. */
int32_t xr_batch_ingest_state(xr_batch* b, const int16_t* owner_dev, const uint64_t* legal_dev, const int32_t* cum_dev, void* stream);
int32_t xr_batch_pack_state(xr_batch* b, uint8_t* rows_dev, int64_t row_bytes, int32_t region_base, void* stream);
int32_t xr_batch_expand_state(xr_batch* b, const uint8_t* rows_dev, int64_t row_bytes, int32_t n_rows, float* head_out_dev, int64_t head_stride,
                              int32_t* nlegal_out_dev, int32_t* region_out_dev, void* stream);

/* Whole-order re-route, the step of the reference's two other env contracts: the A3C env answers the simulator with
 * a complete net list (baseline/A3C/utils.py:305-307, Response.net_list of net_ordering.proto v2 field 2) and the
 * MCTS dispatcher re-routes the region from scratch with `routed_nets + unrouted_nets` after every selection
 * (baseline/xroute/trainer4/dispatcher.py:113-118).  Every env restores its assigned region's initial state and
 * routes orders_dev[e*stride + 0..] (int32, 1-based net ids, a value <= 0 ends the list; stride >= k_max) in that
 * order, in one launch.  Afterwards XR_FETCH_CUM holds the final cumulative metrics, XR_FETCH_DELTA / REWARD the
 * totals over the whole order (cum - initial), XR_FETCH_STATUS the OR over the routed nets, XR_FETCH_PATH_LEN /
 * SWEEPS the sums, XR_FETCH_DONE whether every net was routed.  Illegal entries (out of range, repeated) are skipped and
 * flagged XR_ENV_BAD_ACTION.  net_stats_dev: NULL or int32[n_envs][stride][4], row = net id - 1:
 * {d_violation, d_wirelength, d_via} of that net's route in this order (the simulator's `metrics_delta`, proto v2
 * field 13) and a counter incremented once per route (`count_map`, field 12); rows of nets not routed are left
 * untouched, the caller zeroes the buffer when an episode starts. */
int32_t xr_batch_route_order(xr_batch* b, const int32_t* orders_dev, int32_t stride, int32_t* net_stats_dev,
                             void* stream);

/* Placement of the step kernel for the loaded regions: resident workgroups per CU as the HIP runtime computes it
 * (hipOccupancyMaxActiveBlocksPerMultiprocessor) and LDS bytes per workgroup (dynamic + static).  ispd18_test1-sized
 * regions are laid out for 4 workgroups per CU (4 x 39.9 KB of the 160 KB); a build that loses that is slower by a
 * quarter, so the tests check it. */
int32_t xr_batch_route_occupancy(xr_batch* b, int32_t* workgroups_per_cu, int64_t* lds_bytes_per_workgroup);

/* Duration in milliseconds (HIP events on the library's internal stream) of the net-plane writer kernel that the
 * last xr_batch_step_observe launched in XR_OBS_SPLIT mode; blocks until that kernel has finished.  *mode_out = the
 * mode that call ran in (XR_OBS_FUSED / XR_OBS_SPLIT); *writer_ms = 0 for XR_OBS_FUSED. */
int32_t xr_batch_observe_timing(xr_batch* b, int32_t* mode_out, float* writer_ms);

/* BASELINE config "random net-order policy": actions_dev[e] = a uniformly chosen legal net of env e
 * (1-based; 0 when the env is done), from a counter-based hash of (seed, e, step count). */
int32_t xr_batch_random_actions(xr_batch* b, int32_t* actions_dev, uint64_t seed, void* stream);

/* Replaces build_3Dgrid on the current state (baseline/build_3Dgrid.py:224-270, called at
 * baseline/baseline_utils.py:422-423,469-470): fp32 observation [2+7K, Z, Y, X] of envs
 * [env_lo, env_hi) written at out_dev + (e-env_lo)*env_stride (floats); K = nlegal[e]. */
int32_t xr_batch_observation(xr_batch* b, float* out_dev, int64_t env_stride, int32_t env_lo,
                             int32_t env_hi, void* stream);

int32_t xr_batch_fetch(xr_batch* b, int32_t what, void* dst_dev, size_t dst_bytes, void* stream);

/* Env-state restore: the inverse of xr_batch_fetch for the arrays that ARE the state of the env slots — XR_FETCH_OWNER, _LEGAL,
 * _NLEGAL, _CUM, _DELTA, _REWARD, _DONE, _STATUS, _PATH_LEN, _HASH, _REGION, _REPLAY, _ENV_STEPS, _RECORD (any other selector:
 * XR_ERR_INVALID).  src_dev: a DEVICE buffer or pinned host memory of exactly the array's size; async on `stream`.  The
 * reference never checkpoints its env (the state lives in the simulator process; its agents do: baseline/DQN/DQN.py:236-242):
 * here the whole batch state is a handful of device arrays, so a dump (fetch) / restore (store) pair is the env checkpoint —
 * a batch restored into a twin created with the same config and regions continues bit-identically (hash chains included). */
int32_t xr_batch_store(xr_batch* b, int32_t what, const void* src_dev, size_t src_bytes, void* stream);

/* ---- env groups: step subsets of the slots independently, each on its own stream --------------- */
/* The reference never steps its envs in lock-step: A3C runs 8 workers with a simulator port each (baseline/A3C/discrete_A3C.py:246-247),
 * MCTS 32 Ray workers (baseline/xroute/net_order.py:34), trainer4 N server processes (baseline/xroute/trainer4/launcher.sh:10-12).  Every
 * per-env state lives in per-env rows and the region rotation and the built-in random policy are functions of the env's own counters, so
 * an env's trajectory depends on its own action sequence only: any interleaving of group steps equals the lock-step batch, env by env.
 *
 * xr_batch_set_groups     declares a partition of the slots: group g = slots [bounds_host[g], bounds_host[g + 1]); n_groups + 1 strictly
 *                         ascending values from 0 to n_envs (no empty group), 1 <= n_groups <= XR_MAX_GROUPS.  n_groups == 1 is the
 *                         default (one group = the whole batch).  It may allocate and synchronise: no work of the batch may be in flight
 *                         when it is called.  A reload of the regions keeps the partition.
 * xr_batch_step_group     steps envs [lo, hi) of `group`: actions_dev[i] belongs to env lo + i.  out_dev == NULL: route only, like
 *                         xr_batch_step.  Else also the observation of env lo + i at out_dev + i*env_stride, byte-identical to
 *                         xr_batch_step_observe (the queue form where the batch takes it, else the fused form; never the split form or
 *                         the helper writers, whose internal stream belongs to the batch).  flags & XR_GROUP_INPLACE: the in-place form
 *                         of xr_batch_step_observe_inplace, its validity tracked per group (a group's buffer is valid after a step of
 *                         that group, or an xr_batch_observation that covered the group, into it).  Any whole-batch call that changes
 *                         state invalidates every group's buffer; a group step invalidates the batch-wide one (the next
 *                         xr_batch_step_observe_inplace writes everything).
 * xr_batch_random_actions_group   xr_batch_random_actions for envs [lo, hi): actions_dev[i] for env lo + i (the same action env lo + i
 *                         gets from the whole-batch call at the same env_steps).
 * xr_batch_fetch_group    xr_batch_fetch of the group's rows of a per-env array: XR_FETCH_RECORD, _REWARD, _DONE, _NLEGAL, _STATUS, _LEGAL,
 *                         _DELTA, _CUM, _PATH_LEN, _PATH, _OWNER, _HASH, _REGION, _SWEEPS, _REPLAY, _ENV_STEPS (batch-wide selectors:
 *                         XR_ERR_INVALID); dst_bytes must equal the slice's size exactly (else XR_ERR_RANGE).
 *
 * Concurrency contract.  Host calls on one batch stay serialised, as everywhere.  Device work of DIFFERENT groups may run concurrently on
 * different streams (they share no queue counters, unit lists, route orders or rows; the persistent step launch never has a workgroup
 * wait for another, so launches sized for the whole chip may share it).  Work of one group is ordered by the caller (one stream per group,
 * or events).  A whole-batch call must be ordered after all outstanding group work (and a group step after outstanding whole-batch work). */
#define XR_MAX_GROUPS 64
#define XR_GROUP_INPLACE 1
int32_t xr_batch_set_groups(xr_batch* b, const int32_t* bounds_host, int32_t n_groups);
int32_t xr_batch_step_group(xr_batch* b, int32_t group, const int32_t* actions_dev, float* out_dev, int64_t env_stride, int32_t flags,
                            void* stream);
int32_t xr_batch_random_actions_group(xr_batch* b, int32_t group, int32_t* actions_dev, uint64_t seed, void* stream);
int32_t xr_batch_fetch_group(xr_batch* b, int32_t group, int32_t what, void* dst_dev, size_t dst_bytes, void* stream);

/* ---- uint8 observations: the same grid at one byte a value ------------------------------------- */
/* Every value of the observation is a small integer: planes 0 and the 7K net planes hold 0 or 1, plane 1 the 1-based net ids (at most
 * the region's n_nets).  These calls write byte i of an env's row = (uint8) of float i of the fp32 observation of the same state
 * (xr_batch_observation / xr_batch_step_observe), for i < (2+7K)*N, in the same [2+7K, Z, Y, X] layout; bytes past (2+7K)*N are never
 * written.  A quarter of the bytes: the step's write stream shrinks to match.
 *   Requirements: every loaded region has n_nets <= 255 (else XR_ERR_RANGE, the batch untouched); out_dev 16-byte aligned and env_stride
 *   (BYTES) a multiple of 16 (else XR_ERR_INVALID); env_stride >= (2+7*k_max)*n_max (else XR_ERR_RANGE).  Recommended stride:
 *   (2+7*k_max)*n_max rounded up to 128 bytes (n_max as xr_batch_sizes reports it).
 * xr_batch_step_observe_u8  the step of xr_batch_step_observe (group == -1: the whole batch) or xr_batch_step_group (group >= 0: env group
 *                           `group`, actions_dev / out_dev rows start at the group's first slot), with the uint8 observation of the new
 *                           state.  The step side is identical to the fp32 calls (records, hash chains, rotation, env_steps, router).  It
 *                           always runs the queue form (XR_OBS_QUEUE): obs_mode, obs_helper_blocks and stream_per_region do not apply.
 *                           flags & XR_OBS_U8_INPLACE: the in-place form (xr_batch_step_observe_inplace), valid when out_dev / env_stride
 *                           received the previous uint8 observation of these slots; validity is tracked per (pointer, stride, dtype) and
 *                           follows the fp32 rules for whole-batch and group calls (an fp32 write never validates a uint8 buffer, nor the
 *                           reverse).  Other flag bits: XR_ERR_INVALID.  xr_batch_observe_timing reports XR_OBS_QUEUE (| 16 in place).
 *                           Regions whose N % 16 != 0 keep two bits per node of one net in the step kernel's LDS: a region too large for
 *                           that (~(n_max / 4) bytes beyond the router's LDS) is refused with XR_ERR_RANGE.
 * xr_batch_observation_u8   build_3Dgrid of the current state of envs [env_lo, env_hi) as bytes (xr_batch_observation's twin). */
#define XR_OBS_U8_INPLACE 1
int32_t xr_batch_step_observe_u8(xr_batch* b, int32_t group, const int32_t* actions_dev, uint8_t* out_dev, int64_t env_stride, int32_t flags,
                                 void* stream);
int32_t xr_batch_observation_u8(xr_batch* b, uint8_t* out_dev, int64_t env_stride, int32_t env_lo, int32_t env_hi, void* stream);

/* ---- lookahead: what every candidate net would cost, without stepping ---- */
/* From the state every env is in now: the metric deltas, status and reward xr_batch_step would publish for each net the env may still
 * pick — the one-ply expansion of the reference's MCTS trainer (baseline/xroute/trainer4/dispatcher.py:113-118 re-routes the region from
 * scratch per selection), the greedy cost baseline, the exact one-step target of a DQN.  Every (env, candidate) pair is routed by the same
 * router the step takes (xr_config.router, dial_mult, the XR-Maze v2 knobs and loaded guides included) in a throw-away copy of the slot.
 *   group            -1: the whole batch, rows [0, n_envs).  >= 0: that env group (xr_batch_set_groups); rows start at the group's first
 *                    slot, as in xr_batch_step_observe_u8, and the work is enqueued on `stream` only.
 *   cand_mask_dev    NULL: every legal net.  Else uint64 [rows][legal_words]: the candidates of an env are legal & mask (bits beyond the
 *                    region's nets are ignored).
 *   out_dev          int32 [rows][k_cap][4], k_cap >= k_max.  The entry of net n (1-based) is at index n - 1: {d_violation, d_wirelength,
 *                    d_via, status} = exactly the delta and the XR_ENV_* status xr_batch_step would publish for this env if n were its
 *                    action now.  Every entry that is not a candidate (net not legal, masked out, index beyond the region's nets) is
 *                    {0, 0, 0, -1}.  An env that is done (no legal net) gets only such rows: lookahead does not look through an auto-reset.
 *   reward_out_dev   NULL, or double [rows][k_cap]: the trainers' reward -(w_violation*dv + w_via*dvia + w_wirelength*dwl) with the bits
 *                    the step's record would carry; -inf for non-candidates, so an arg-max over a row is the greedy action.
 * Errors (the batch is untouched after any of them): XR_ERR_INVALID null b / out_dev, or a group outside -1 .. n_groups - 1; XR_ERR_STATE
 * before xr_batch_load_regions; XR_ERR_RANGE k_cap < k_max; XR_ERR_RANGE for batches whose distance field does not fit LDS (the
 * HBM-scratch router forms, force_scratch_field included) and for stream_per_region: the shadow slots have no scratch rows of their own.
 * Contract.  Lookahead never synchronises: it only enqueues on `stream` (a planning kernel, then one persistent launch).  It may allocate
 * its private memory (shadow slots: about workgroups x (2*n_max + 4*path_cap) bytes, a task list, counters) on the first call, per batch
 * and per group.  It leaves NO TRACE in the batch: every array xr_batch_fetch returns (owner, legal, cum, delta, reward, done, status, path,
 * path_len, hash, region, replay, env_steps, steps, sweeps, records, ...) is only read, and the validity of the in-place observation
 * buffers (fp32 and uint8, batch-wide and per group) is kept — an xr_batch_step_observe_inplace after a lookahead still takes the in-place
 * path.  Lookaheads of DIFFERENT groups may be in flight at once on different streams, under the concurrency contract of
 * xr_batch_step_group (each group has shadow slots and counters of its own; no workgroup waits for another); a lookahead of one group and
 * steps of the SAME group are ordered by the caller, and so are a whole-batch lookahead and any step. */
int32_t xr_batch_lookahead(xr_batch* b, int32_t group, const uint64_t* cand_mask_dev, int32_t* out_dev, int32_t k_cap, double* reward_out_dev,
                           void* stream);

/* ---- rollouts: every env's episode played to its end, without stepping ---- */
/* From the state every env is in now: what the whole rest of the episode costs under a given continuation, n_rollouts continuations per
 * env — the many-ply expansion of the reference's MCTS trainer (baseline/xroute/trainer4/dispatcher.py:113-118), a Monte-Carlo value
 * estimate, the "best of R random orderings" net-ordering baseline.  For every row (an env of the whole batch or of one env group, as in
 * xr_batch_lookahead) and every r in [0, n_rollouts): copy the env's state into a throw-away shadow slot, route the prefix, continue under
 * `policy` — every route by the same router the step takes (xr_config.router, dial_mult, the XR-Maze v2 knobs and loaded guides included).
 *   group            -1: the whole batch, rows [0, n_envs).  >= 0: that env group; rows start at the group's first slot, and the work is
 *                    enqueued on `stream` only.
 *   n_rollouts       1 .. XR_ROLLOUT_MAX continuations per env.
 *   policy           XR_ROLLOUT_STOP: play the prefix only.  XR_ROLLOUT_RANDOM: after the prefix, the built-in random policy until no net
 *                    is left (or max_plies) with seed_r = seed + r * 0x9E3779B97F4A7C15 (mod 2^64): at every ply the net
 *                    xr_batch_random_actions(seed_r) would choose for THIS env from the shadow state (keyed by the global env index and
 *                    the shadow's env_steps, which a real route advances and a rejected action does not).  Rollout r of env e is bit for
 *                    bit what a twin batch in the same state does when stepped to the end with xr_batch_random_actions(seed_r).
 *   prefix_dev       NULL, or int32 [rows][n_rollouts][prefix_stride] of 1-based net ids, a value <= 0 ends a list.  An entry that is not
 *                    legal at that point is skipped and flagged XR_ENV_BAD_ACTION in the rollout's status, as xr_batch_route_order treats
 *                    it; a skipped entry costs no ply.  Once no net is left the rest of a list is ignored.
 *   max_plies        0: until no legal net is left.  > 0: stop after that many real routes, the prefix's included.
 *   out_dev          int32 [rows][n_rollouts][8]: {d_violation, d_wirelength, d_via (cumulative at the end minus cumulative now), status
 *                    (OR of the XR_ENV_* bits of every route and every skipped entry), plies (real routes made), nlegal_end, path_len_sum,
 *                    0}.
 *   return_out_dev   NULL, or double [rows][n_rollouts]: the sum of the per-step rewards, added in step order in double from 0.0.
 *   hash_out_dev     NULL, or uint64 [rows][n_rollouts]: the env's hash chain (XR_FETCH_HASH) continued over the rollout's routes.
 *   order_out_dev    NULL, or int32 [rows][n_rollouts][k_cap]: the nets routed, in order; entries past `plies` are 0.  k_cap >= k_max is
 *                    required only when order_out_dev is given.
 * An env that is done (no legal net) gets the empty rollout — rollouts never look through an auto-reset: {0, 0, 0, 0, 0, 0, 0, 0}, return
 * 0.0, hash = the env's current hash, order all 0.  (A rollout that makes no route from a live env — XR_ROLLOUT_STOP without a usable
 * prefix — is the same except nlegal_end = the env's nlegal, and XR_ENV_BAD_ACTION if entries were skipped.)
 * Errors (the batch is untouched after any of them): XR_ERR_INVALID null b / out_dev, a group outside -1 .. n_groups - 1, an unknown
 * policy, prefix_dev with prefix_stride < 1, a negative max_plies; XR_ERR_STATE before xr_batch_load_regions; XR_ERR_RANGE n_rollouts
 * outside 1 .. XR_ROLLOUT_MAX, k_cap < k_max with order_out_dev, rows x n_rollouts beyond 31 bits; XR_ERR_RANGE for the HBM-scratch router
 * forms (force_scratch_field included) and for stream_per_region, for lookahead's reason.
 * Contract, the same as lookahead's.  A rollout never synchronises: it only enqueues on `stream` (one persistent launch; tasks are claimed
 * from a counter that the previous launch on the pool zeroed).  It may allocate its private memory on the first call, per batch and per
 * group (it plays in lookahead's shadow slots, with claim counters of its own).  It leaves NO TRACE in the batch: every array
 * xr_batch_fetch returns is only read, and the validity of the in-place observation buffers (fp32 and uint8, batch-wide and per group) is
 * kept.  Rollouts of DIFFERENT groups may be in flight at once on different streams; within one group (or for the whole batch) rollouts,
 * lookaheads and steps are ordered by the caller. */
#define XR_ROLLOUT_STOP    0   /* play the prefix only */
#define XR_ROLLOUT_RANDOM  1   /* after the prefix: the built-in random policy until no net is left (or max_plies) */
#define XR_ROLLOUT_MAX     4096
int32_t xr_batch_rollout(xr_batch* b, int32_t group, int32_t n_rollouts, int32_t policy, uint64_t seed,
                         const int32_t* prefix_dev, int32_t prefix_stride, int32_t max_plies,
                         int32_t* out_dev, double* return_out_dev, uint64_t* hash_out_dev,
                         int32_t* order_out_dev, int32_t k_cap, void* stream);

/* ---- peek: the state after a line of play, packed, without stepping ---- */
/* From the state every env is in now: the STATE the env would be in after a given line of play, n_lines lines per env, as the packed
 * state row of xr_batch_pack_state — what xr_batch_expand_state turns into the head rows xr_batch_step_compact writes and into the nlegal /
 * region arrays xr_agent_actor takes, so that a network can be asked about a state the env is not in (a critic value for every successor,
 * a learned tree prior).  For every row (an env of the whole batch or of one env group, exactly as in xr_batch_rollout) and every line l
 * in [0, n_lines): copy the env's state into a throw-away shadow slot and route the line's prefix there under xr_batch_rollout's prefix
 * rules — every route by the same router the step takes.  Nothing continues after the prefix: the policy is always "stop".
 *   group            -1: the whole batch, rows [0, n_envs).  >= 0: that env group; rows start at the group's first slot, and the work is
 *                    enqueued on `stream` only.
 *   n_lines          1 .. XR_PEEK_MAX lines per env.
 *   prefix_dev       NULL, or int32 [rows][n_lines][prefix_stride] of 1-based net ids, a value <= 0 ends a list.  An entry that is not
 *                    legal at that point is skipped and flagged XR_ENV_BAD_ACTION in the line's status; a skipped entry costs no ply.
 *                    Once no net is left the rest of a list is ignored.
 *   max_plies        0: the whole list.  > 0: stop after that many real routes.
 *   rows_out_dev     uint8 [rows][n_lines][row_bytes], 8-byte aligned, row_bytes a multiple of 8 and >= xr_batch_state_row_bytes: row
 *                    (row * n_lines + l) is the packed state row of the shadow slot after the line, in xr_batch_pack_state's format
 *                    (int32 region + region_base | nlegal | legal_words | occ_words, uint64 legal[legal_words], uint64
 *                    occ[occ_words]) — byte-identical to what xr_batch_pack_state(region_base) writes for a twin env that really stepped
 *                    the line's legal nets in order.  Bytes of a row beyond 16 + 8 * (legal_words + occ_words) are not written.
 *   region_base      added to the env's region index in the row's header, as in xr_batch_pack_state.
 *   out_dev, return_out_dev, hash_out_dev, order_out_dev, k_cap
 *                    [rows][n_lines]...: bit for bit what xr_batch_rollout(..., XR_ROLLOUT_STOP, ...) writes for the same arguments
 *                    (return / hash / order may be NULL; k_cap >= k_max is required only with order_out_dev).
 * A line that makes no real route (prefix_dev == NULL, an empty list, a list of illegal entries only, a done env) writes the row of the
 * env's current state and the empty rollout record — peek never looks through an auto-reset.  Every output entry is written exactly once
 * per call.
 * Errors (the batch is untouched after any of them): XR_ERR_INVALID null b / rows_out_dev / out_dev, rows_out_dev not 8-byte aligned or
 * row_bytes % 8 != 0, a group outside -1 .. n_groups - 1, prefix_dev with prefix_stride < 1, a negative max_plies; XR_ERR_STATE before
 * xr_batch_load_regions; XR_ERR_RANGE n_lines outside 1 .. XR_PEEK_MAX, row_bytes < xr_batch_state_row_bytes, k_cap < k_max with
 * order_out_dev, rows x n_lines beyond 31 bits; XR_ERR_RANGE for the HBM-scratch router forms (force_scratch_field included) and for
 * stream_per_region, for lookahead's reason.
 * Contract, rollout's word for word.  A peek never synchronises: it only enqueues on `stream` (one persistent launch; tasks are claimed
 * from a counter that the previous launch on the pool zeroed).  It may allocate its private memory on the first call, per batch and per
 * group: it plays in lookahead's shadow slots and claims from the rollout's claim counters (two alternating banks, no memset per call;
 * peeks and rollouts on one pool are ordered by the caller anyway).  It leaves NO TRACE in the batch: every array xr_batch_fetch returns
 * is only read, and the validity of the in-place observation buffers (fp32 and uint8, batch-wide and per group) is kept.  Peeks of
 * DIFFERENT groups may be in flight at once on different streams; within one group (or for the whole batch) peeks, rollouts, lookaheads
 * and steps are ordered by the caller. */
#define XR_PEEK_MAX 4096   /* = XR_ROLLOUT_MAX */
int32_t xr_batch_peek(xr_batch* b, int32_t group, int32_t n_lines,
                      const int32_t* prefix_dev, int32_t prefix_stride, int32_t max_plies,
                      uint8_t* rows_out_dev, int64_t row_bytes, int32_t region_base,
                      int32_t* out_dev, double* return_out_dev, uint64_t* hash_out_dev,
                      int32_t* order_out_dev, int32_t k_cap, void* stream);

/* ---- branch: env slots take other slots' state, on the device ---- */
/* The primitive of every search that keeps more than one line of play (beam search, the tree expansion of the reference's MCTS trainer,
 * baseline/xroute/trainer4/dispatcher.py:113-118): slot i continues from the state slot parent[i] is in now.  A permuted copy of the
 * per-env rows that never leaves device memory; the copied state is valid by construction, so nothing is checked on the host.
 *   group            -1: the whole batch, rows [0, n_envs).  >= 0: that env group; rows AND parent indices are relative to the group's
 *                    first slot, as in xr_batch_lookahead, and the work is enqueued on `stream` only.
 *   parent_dev       int32 [rows]: row i takes the state of row parent[i].  parent[i] < 0 or parent[i] == i: the slot keeps its state.
 *                    parent[i] >= rows (out of range — for a group, also an index that is valid for the batch but outside the group):
 *                    the slot keeps its state and gets XR_ENV_BAD_ACTION OR-ed into its status (XR_FETCH_STATUS) and its record's
 *                    status; nothing else of it changes.
 * Gather semantics: every read sees the state BEFORE the call, whatever the map is — a swap, a cycle, a chain, a fan-out of one slot to
 * many (also from a slot that is itself overwritten, or flagged: its children see it without the flag); the map need not be injective.
 * After the call every per-env row xr_batch_fetch returns for slot i — owner, legal, nlegal, cum, delta, reward, done, status, path,
 * path_len, hash, region, replay, env_steps, record, sweeps, touched, whole rows — is byte-identical to what it returned for slot
 * parent[i] before the call.  total_steps, the measured net classes and the regions are untouched.  A slot may take the state of a slot
 * that plays another region: it then plays that region (region and replay travel with it).  A branched slot is a full env: stepped on, it
 * does bit for bit what its parent would have done (hash chain, rotation, auto-reset); xr_batch_random_actions stays keyed by the slot's
 * own index.
 * Works for every router variant, the HBM-scratch forms (force_scratch_field included) and stream_per_region too: the router scratch is
 * clean between routes, so the rows above are all the state a slot has.
 * Contract.  A branch never synchronises: it only enqueues on `stream` (two launches: the parents of overwritten parents go to a staging
 * pool, then every moved slot is written from its untouched parent or from staging; no launch reads and writes the same slot, and no
 * workgroup ever waits for another).  It may allocate its private memory on the first call, per batch and per group: one staging row of
 * every array above per row of the caller, rows x (2 n_max + 4 path_cap + 8 legal_words + 125) bytes, rounded up to 16 per array.
 * Observation validity is dropped the way a state-changing call drops it: a whole-batch call drops every in-place buffer's (fp32 and
 * uint8, batch-wide and per group), a group call that group's and the batch-wide one.  Branches of DIFFERENT groups may be in flight at
 * once on different streams under the xr_batch_step_group concurrency contract (each group has its own staging); within one group (or
 * for the whole batch) branches, steps, lookaheads and rollouts are ordered by the caller.
 * Errors (the batch is untouched after any of them): XR_ERR_INVALID null b / parent_dev, or a group outside -1 .. n_groups - 1;
 * XR_ERR_STATE before xr_batch_load_regions; XR_ERR_NOMEM when the staging pool cannot be allocated. */
int32_t xr_batch_branch(xr_batch* b, int32_t group, const int32_t* parent_dev, void* stream);

/* ---- tree search: MCTS over net orderings, the tree on the device ---- */
/* The search of the reference's MuZero / MCTS agent (baseline/xroute/self_route.py:341-371, 482-568, 571-613, re-routing per selection in
 * trainer4/dispatcher.py:113-118) as ONE enqueue-only call: pUCT selection, evaluation by rollouts (xr_batch_rollout's kernel) and backup
 * all run on the device, n_waves x n_par simulations per row, no host round trip per simulation.  A row is an env of the whole batch
 * (group -1) or of one env group, as in xr_batch_lookahead.  "XR-Tree v1" (build-defined, as XR-Maze is):
 *   Nodes.   One tree per row, rebuilt on every call.  A node is a set of nets routed after the env's current state, in path order; its
 *            legal set is the env's legal set minus the nets of its path (selection needs no env state); a node with an empty legal set
 *            is terminal.  Expanding a node allocates one child per legal net: one contiguous block in ascending net order out of the
 *            row's pool of node_cap nodes.  A block that does not fit leaves the node unexpanded and sets XR_TREE_POOL_FULL in the row's
 *            info.  The root (node 0) is expanded when the call starts.  Per node: real visits N, pending visits V, value sum W (double),
 *            prior P (double).
 *   Prior.   prior_dev: NULL, or fp32 [rows][k_cap] weights per net (index net - 1); an entry that is not finite or is < 0 counts as 0.
 *            P(child) = w[net] / S, S = the sum of w over the parent's legal nets, added in ascending net order in double; S == 0 or
 *            prior_dev NULL: P = 1 / count.  Softmax is the caller's business.
 *   Table.   E[n] = (log((n + c_base + 1) / c_base) + c_init) * sqrt(n), computed on the HOST in double for n = 0 .. n_waves * n_par and
 *            uploaded with the call (the kernels call no log and no sqrt); xr_tree_exploration_table returns the same numbers.
 *   Waves.   A search is n_waves waves of n_par simulations; a wave is three enqueues: select, the rollout launch, backup.
 *   Select.  Per row the lanes j = 0 .. n_par - 1 descend one after the other: from the root to the best child for as long as the node is
 *            expanded; a lane stops at an unexpanded or terminal node, and expands an unexpanded non-terminal one if the pool has room.
 *            Its path is the nets from the root to that node; it then adds 1 to V of every node of the path, the root included.  Score
 *            of child c under parent p, with n = N + V:  u = (E[n_p] * P_c) / (double)(n_c + 1);  v = (N_c > 0 && max > min) ?
 *            (W_c / N_c - min) / (max - min) : 0.0;  score = u + v.  The best child is the maximum under >, so a tie goes to the lowest
 *            net.  Every operation is one IEEE double operation, rounded on its own (no contraction, no fast-math).
 *   Evaluate. Simulation (w, j) is rollout j of one rollout launch over the rows: n_rollouts = n_par, XR_ROLLOUT_RANDOM, max_plies 0,
 *            seed_w = seed + w * 0xD1B54A32D192ED03 (mod 2^64), the prefix = the wave's paths.  G is the rollout's return: the return of
 *            the whole line from the env's current state (siblings share everything above them, so ordering them by G is ordering them
 *            by reward + value); the rollout's order row is the simulation's complete ordering.
 *   Backup.  Per row the simulations are taken in lane order (the order of the double additions is part of the spec).  On every node of
 *            the path: N += 1, V -= 1, W += G.  Then min = fmin(min, G), max = fmax(max, G), and if G > best (strictly: the first wins)
 *            best = G and the best order becomes the order row.  min / max / best start at +inf / -inf / -inf.
 *   Done rows. A row whose env is done (no legal net) runs no simulation — tree search never looks through an auto-reset: visits all 0,
 *            values all -inf, info all 0, best order all 0, best return -inf, every path empty, every return 0.0.
 *   n_waves, n_par   >= 1; n_par <= XR_ROLLOUT_MAX, n_waves * n_par <= 65536.
 *   node_cap         >= 1 nodes per row, the root included (1 + (n_waves * n_par + 1) * k_max always suffices: the root's block and
 *                    one per simulation).
 *   visits_out_dev   int32 [rows][k_cap]: N of the root's child of net n at index n - 1; 0 for every non-candidate.
 *   value_out_dev    double [rows][k_cap]: W / N of that child, -inf where N == 0.
 *   info_out_dev     int32 [rows][4] = {simulations, nodes_used (the root included), max_depth (the longest path), flags}.
 *   best_order_out_dev / best_return_out_dev   NULL, or int32 [rows][k_cap] / double [rows]: the best line any simulation saw.
 *   paths_out_dev / returns_out_dev   NULL, or int32 [rows][n_waves * n_par][k_cap] (ended by 0) / double [rows][n_waves * n_par]: every
 *                    simulation's path and G, in (w, j) order.
 * Cuts: no tree reuse between calls, no Dirichlet noise, no network inside the tree, no discounting, no HBM-scratch forms.
 * Contract, the same as the rollout's.  A tree search never synchronises: it only enqueues on `stream` (a reset launch, the table's
 * copy, then select / rollout / backup per wave; no workgroup waits for another one).  It may allocate its private memory
 * on the first call, per batch and per group, and again when a call needs more than any before it:
 * rows x (40 node_cap + 40 + n_par x (8 k_cap + 40)) bytes, each of its six arrays rounded up to 16, plus 8 x (n_waves x n_par + 1) bytes per distinct (c_init, c_base) for the table, plus
 * lookahead's shadow slots and the rollout's claim counters where the caller has not used them yet.  It leaves NO TRACE in the batch: it
 * plays in lookahead's shadow slots, every array xr_batch_fetch returns is only read, and the validity of the in-place observation
 * buffers (fp32 and uint8, batch-wide and per group) is kept.  Searches of DIFFERENT groups may be in flight at once on different
 * streams; within one group (or for the whole batch) searches, rollouts, lookaheads, branches and steps are ordered by the caller.
 * Errors (the batch is untouched after any of them): XR_ERR_INVALID null b / visits_out_dev / value_out_dev / info_out_dev, a group
 * outside -1 .. n_groups - 1, n_waves < 1, n_par < 1, a c_init that is not finite, a c_base that is not > 0 and finite; XR_ERR_STATE
 * before xr_batch_load_regions, or where the kernels are not linked; XR_ERR_RANGE n_par > XR_ROLLOUT_MAX, n_waves * n_par > 65536,
 * node_cap < 1, k_cap < k_max, and for the HBM-scratch router forms (force_scratch_field included) and stream_per_region, for the
 * rollout's reason; XR_ERR_NOMEM when the private memory cannot be allocated.
 * xr_tree_exploration_table (host only, no batch, no device): E[0 .. n] into out_host[n + 1].  XR_ERR_INVALID for a null out_host, n < 0
 * or the knobs refused above. */
#define XR_TREE_POOL_FULL 1
#define XR_TREE_MAX_SIMS 65536
int32_t xr_tree_exploration_table(double c_init, double c_base, int32_t n, double* out_host);
int32_t xr_batch_tree_search(xr_batch* b, int32_t group, int32_t n_waves, int32_t n_par, uint64_t seed,
                             const float* prior_dev, int32_t node_cap, double c_init, double c_base,
                             int32_t* visits_out_dev, double* value_out_dev, int32_t k_cap, int32_t* info_out_dev,
                             int32_t* best_order_out_dev, double* best_return_out_dev,
                             int32_t* paths_out_dev, double* returns_out_dev, void* stream);

/* ---- weighted net sampling: actions, rollouts and tree simulations that follow per-net weights ---- */
/* One more built-in policy beside the uniform pick of xr_batch_random_actions: a legal net drawn with probability proportional to a
 * caller-supplied weight per net — the Categorical(action_probs) sample of the reference's PPO (baseline/PPO/PPO.py:124-146) and the
 * learned policy under which its MCTS plays simulations (baseline/xroute/self_route.py:482-568), for any caller that has per-net scores
 * (an actor head's logits, lookahead rewards, elite statistics of earlier rollouts), without leaving the device loop.  Weights are
 * integers and fixed for the call, so a whole rollout is a Plackett-Luce sample of an ordering.  "XR-Pick v1" (build-defined, exact in
 * integers, bit for bit reproducible on the host):
 *   Inputs.   A row's legal set, its env_steps, the global env index e, a 64-bit seed, and a weight row int32 w[k_cap] with net n at index
 *             n - 1.
 *   Effective weight.  q(n) = 0 if w <= 0, else min(w, XR_WEIGHT_MAX); XR_WEIGHT_MAX = 1 << 24, so the sum over any 64 nets fits 31 bits
 *             and only the total needs 64.  Entries of nets that are not legal, or lie beyond the region's nets, are never read into the
 *             result.
 *   Hash.     r = splitmix64(seed ^ splitmix64(e * 0x100000001B3 + env_steps)) (mod 2^64): the same bits xr_batch_random_actions uses.
 *   Pick.     L = the number of legal nets, S = the sum of q(n) over them.  L == 0: the pick is 0.  S == 0: the uniform pick, legal net
 *             number r % L in ascending order.  Otherwise t = r % S, and the pick is the lowest legal net whose running sum of q over
 *             the legal nets in ascending order exceeds t.  Everything is integer: any summation order gives the same answer.
 *   Consequences.  All effective weights 1 gives exactly the net xr_batch_random_actions returns.  A net with q = 0 is picked only when
 *             every legal net has q = 0.
 * Weights are device data and are never validated on the host: the clamp is the validation.
 * xr_batch_weighted_actions     actions_dev[i] = the XR-Pick of row i from weights_dev[i][0 .. k_cap), k_cap >= k_max.  group -1: the whole
 *                               batch; >= 0: that env group, rows start at the group's first slot.  It only enqueues on `stream`.  Keyed
 *                               by the global env index: sharding- and group-invariant like xr_batch_random_actions.  XR_ERR_INVALID null
 *                               b / weights_dev / actions_dev, a group outside -1 .. n_groups - 1; XR_ERR_STATE before
 *                               xr_batch_load_regions, or where the kernel is not linked; XR_ERR_RANGE k_cap < k_max.
 * xr_batch_rollout_weighted     xr_batch_rollout with one more policy.  policy XR_ROLLOUT_STOP / XR_ROLLOUT_RANDOM: exactly what
 *                               xr_batch_rollout does (weights_dev is not looked at).  XR_ROLLOUT_WEIGHTED: after the prefix, at every
 *                               ply the net xr_batch_weighted_actions(seed_r) would choose for THIS env from the shadow state, from the
 *                               weights of the env's row: weights_dev int32 [rows][weights_k_cap], shared by the row's rollouts.  seed_r,
 *                               prefix, max_plies, outputs, done envs, pools, claim counters and the no-trace / concurrency contract are
 *                               the rollout's.  Errors as xr_batch_rollout, and XR_ERR_INVALID null weights_dev with XR_ROLLOUT_WEIGHTED,
 *                               XR_ERR_RANGE weights_k_cap < k_max with it.  xr_batch_rollout itself keeps refusing policy 2.
 * xr_batch_tree_search_weighted XR-Tree v1 unchanged, except that Evaluate runs XR_ROLLOUT_WEIGHTED with sim_weights_dev (int32
 *                               [rows][k_cap], the k_cap of the call).  NULL sim_weights_dev: xr_batch_tree_search exactly.  Errors as
 *                               xr_batch_tree_search.
 * Cuts: the weights are fixed for the call (no per-ply update), one weight row per env (no per-rollout weights), no network in the loop. */
#define XR_ROLLOUT_WEIGHTED 2   /* after the prefix: XR-Pick v1 under the row's weights (xr_batch_rollout_weighted only) */
#define XR_WEIGHT_MAX (1 << 24)
int32_t xr_batch_weighted_actions(xr_batch* b, int32_t group, const int32_t* weights_dev, int32_t k_cap, int32_t* actions_dev, uint64_t seed,
                                  void* stream);
int32_t xr_batch_rollout_weighted(xr_batch* b, int32_t group, int32_t n_rollouts, int32_t policy, uint64_t seed,
                                  const int32_t* prefix_dev, int32_t prefix_stride, int32_t max_plies,
                                  int32_t* out_dev, double* return_out_dev, uint64_t* hash_out_dev,
                                  int32_t* order_out_dev, int32_t k_cap,
                                  const int32_t* weights_dev, int32_t weights_k_cap, void* stream);
int32_t xr_batch_tree_search_weighted(xr_batch* b, int32_t group, int32_t n_waves, int32_t n_par, uint64_t seed,
                                      const float* prior_dev, int32_t node_cap, double c_init, double c_base,
                                      int32_t* visits_out_dev, double* value_out_dev, int32_t k_cap, int32_t* info_out_dev,
                                      int32_t* best_order_out_dev, double* best_return_out_dev,
                                      int32_t* paths_out_dev, double* returns_out_dev,
                                      const int32_t* sim_weights_dev, void* stream);

/* ---- kept trees: a search that continues from the played net's subtree ---- */
/* The standard MCTS saving (the reference's play loop keeps none: baseline/xroute/self_route.py:341-371 builds a new root at every
 * move): after the env has really played net a, the root's child of a and everything below it is a valid tree for the new state.
 * xr_batch_tree_search_keep is xr_batch_tree_search_weighted in every argument it shares with it (sim_weights_dev NULL: the random
 * simulations; the errors, the no-trace contract, the enqueue-only contract and the refusal of the HBM-scratch forms and
 * stream_per_region are the same, every refusal names xr_batch_tree_search_keep), except for what follows.  "XR-Tree v1, kept":
 *   Own memory. Every caller (the whole batch, or one env group) has a kept-tree pool of its own, apart from the pool of the plain
 *            searches: xr_batch_tree_search and xr_batch_tree_search_weighted never disturb a kept tree, and a kept call never disturbs
 *            them.  The pool holds two halves of rows x node_cap nodes (a call re-roots from the half the last call searched in into the
 *            other one), the row states, a key per row, and the wave arrays of the plain search:
 *            rows x (80 node_cap + 40 + 24 + 8 legal_words) bytes for the trees, each of its five arrays rounded up to 16, allocated
 *            when the shape below changes, and rows x n_par x (8 k_cap + 40) bytes of wave arrays that only grow, plus
 *            8 x (XR_TREE_MAX_SIMS + 1) bytes per distinct (c_init, c_base) for the table.
 *   Key.     The key of a row is written at the end of the call's first kernel: the env's env_steps, region, replay and legal words as
 *            they are at that moment, and a valid bit.
 *   played_dev.  NULL: every row is rebuilt (a fresh search that leaves a kept tree behind).  Otherwise int32 [rows]:
 *            played[row] == 0: the env has not moved since the kept tree's call.  The row is kept whole if the key is valid and equals
 *            the env's current env_steps, region, replay and legal words exactly, and the kept root's N plus n_waves * n_par does not
 *            exceed XR_TREE_MAX_SIMS.
 *            played[row] == a > 0: the env has since made exactly one real route, of net a.  The row is re-rooted if all of these
 *            hold: the key is valid; region and replay are equal; env_steps == key.env_steps + 1; bit a is set in the key's legal words;
 *            the env's legal words equal the key's with bit a cleared; the kept root is expanded and has a child of net a; that child's
 *            N plus n_waves * n_par does not exceed XR_TREE_MAX_SIMS.
 *            Otherwise, and for any negative entry, the row is rebuilt exactly as the plain search builds it.  A rebuild is never an
 *            error.  The host rebuilds all rows when rows, the group's first slot, node_cap, k_cap or legal_words differ from the
 *            pool's last call; n_par, n_waves, the knobs and the seed may differ.
 *   Re-rooting (normative, node numbering included).  New node 0 is the old child of a, with net = 0 and P = 1.0.  The new nodes are
 *            then taken in index order, and the children block of every expanded one is appended in its old (ascending net) order: a
 *            breadth-first compaction.  nodes_used is the count; it always fits.  Let r be the slot's reward row (the reward of the step
 *            that played a).  Every copied node gets W' = W - (double)N * r: one multiplication, then one subtraction, each rounded on
 *            its own; N, P, net and count are kept, V is 0.  The row state gets min' = min - r and max' = max - r (infinities stay).
 *            With played == 0 nothing is shifted or renumbered.  In both cases best restarts at -inf, max_depth at 0, and the flags
 *            become XR_TREE_KEPT alone.  A new root that is unexpanded is expanded at the start with this call's prior, as the plain
 *            search does.  A row whose env has no legal net (the played net was the last) is a done row: the empty result, kept {0, 0}.
 *            Kept nodes keep the P they were given: prior_dev of this call serves new expansions only.
 *   Table.   A kept root meets visit counts above n_waves * n_par: kept calls index E[n] for n = 0 .. XR_TREE_MAX_SIMS, computed once
 *            per (c_init, c_base) by the same formula.
 *   Outputs. info = {simulations of this call, nodes_used, max_depth of this call, flags}; visits_out and value_out show the root's
 *            children with the carried visits included, in the current frame.  kept_out_dev: NULL, or int32 [rows][2] = {N of the new
 *            root before this call's simulations, nodes carried}; {0, 0} for a rebuilt row.
 * Cuts: the best line does not carry (best_order and best_return are this call's simulations' alone); one real route per call at
 * most (a row whose env made two is rebuilt); a tree does not follow a branch to another slot. */
#define XR_TREE_KEPT 2
int32_t xr_batch_tree_search_keep(xr_batch* b, int32_t group, const int32_t* played_dev,
                                  int32_t n_waves, int32_t n_par, uint64_t seed, const float* prior_dev, int32_t node_cap,
                                  double c_init, double c_base, int32_t* visits_out_dev, double* value_out_dev, int32_t k_cap,
                                  int32_t* info_out_dev, int32_t* best_order_out_dev, double* best_return_out_dev,
                                  int32_t* paths_out_dev, double* returns_out_dev, const int32_t* sim_weights_dev,
                                  int32_t* kept_out_dev, void* stream);

/* ---- evaluated tree search: leaves valued by the caller's network ---- */
/* The search of the reference's MuZero agent with the network where the reference has it (baseline/xroute/self_route.py:341-371, 482-568):
 * a simulation stops at the selected leaf, the leaf's STATE goes to the caller's evaluator as a packed state row (xr_batch_peek's), and
 * the evaluator's value — plus, optionally, a prior for the leaf's own children — goes back into the tree.  A simulation routes only the
 * nets on its path; nothing is rolled out to the end of the episode.  Three enqueue-only entry points, called in the order
 * open, {leaves, [the caller's evaluator, on the same stream], backup} x waves; no host round trip anywhere.  A row is an env of the whole
 * batch (group -1) or of one env group, as in xr_batch_lookahead.  "XR-Tree v2, evaluated" (build-defined); Nodes, Prior, Table, Select
 * and Backup are XR-Tree v1's (the tree search section above) except for what follows:
 *   Own memory. Every caller (the whole batch, or one env group) has an evaluated-tree pool of its own, apart from the pool of the plain
 *            searches and from the kept-tree pool: none of the three searches disturbs another.  The pool holds one session:
 *            rows x (40 node_cap + 40 + n_par x (4 k_cap + 16) + 8 k_cap + 8 legal_words + 4) bytes, each of its nine arrays (nodes, row
 *            states, paths, line returns, leaf records, best order, legal words, nlegal, prior) rounded up to 16, allocated again when
 *            an open call needs more than any before it, plus 8 x (max_sims + 1) bytes per distinct (c_init, c_base, max_sims) for the
 *            table, plus lookahead's shadow slots and the rollout's claim counters where the caller has not used them yet (the peek
 *            launch plays there).
 * xr_batch_tree_open     starts a session (and ends the pool's last one, whatever state it was in).  It uploads E[0 .. max_sims] (v1's
 *            Table, computed on the host; xr_tree_exploration_table returns the same numbers) and runs one kernel: per row it copies the
 *            env's nlegal and legal words — the SNAPSHOT — and the row of root_prior_dev into the pool, resets the row state exactly as
 *            the plain search does (min / max / best = +inf / -inf / -inf, no node, depth 0, flags 0), and builds the root and expands it
 *            under v1's Prior rule from root_prior_dev (fp32 [rows][k_cap], or NULL: uniform).  Every later kernel of the session reads
 *            the snapshot, never the env's live words, and root_prior_dev is not read again after this call.  A caller who steps the env
 *            (or resets it, or branches into it) between open and the last backup gets unspecified numbers — every access stays in bounds
 *            — and must re-open.  Done rows (no legal net at the open call) get v1's empty result from every backup and take part in
 *            nothing.
 *   n_par            1 .. XR_PEEK_MAX lanes per wave.
 *   max_sims         n_par .. XR_TREE_MAX_SIMS: the simulations the session may run, the last entry of its table.
 *   node_cap         >= 1 nodes per row, the root included (1 + (max_sims + 1) * k_max always suffices).
 *   k_cap            >= k_max: the row length of every per-net array of the session.
 * xr_batch_tree_leaves   one wave, two enqueues (and a device-to-device copy of rows x n_par doubles when return_out_dev is given).
 *   Select.  v1's Select rule word for word: the lanes j = 0 .. n_par - 1 descend one after the other, pending visits V included, the
 *            best child is the maximum under >, a tie goes to the lowest net.  A lane stops at an unexpanded or terminal node.  An
 *            unexpanded non-terminal node — a FRESH leaf — is expanded at select time if the pool has room, its block's P taken from the
 *            open call's row prior under v1's rule.  Select writes paths_out_dev (NULL, or int32 [rows][n_par][k_cap], each list ended
 *            by 0 unless it has k_cap nets) and leaf_out_dev (NULL, or int32 [rows][n_par][2] = {node index, flags}); the flags are
 *            XR_TREE_LEAF_TERMINAL (the path holds every legal net of the snapshot), XR_TREE_LEAF_FRESH (this lane expanded the node
 *            in this wave) or 0 (an unexpanded node a full pool has no room for); a done row has {-1, XR_TREE_LEAF_NONE} and empty paths.
 *   Peek.    One peek launch — xr_batch_peek's kernel through its launcher — with n_lines = n_par, the prefix = the wave's paths,
 *            max_plies 0: rows_out_dev (uint8 [rows][n_par][row_bytes]), out_dev (int32 [rows][n_par][8]) and return_out_dev (NULL, or
 *            double [rows][n_par]) are bit for bit what xr_batch_peek writes for that prefix; row_bytes and region_base are its
 *            arguments.  The tree keeps the line returns for the backup.
 * xr_batch_tree_backup   one enqueue.  value_dev: double [rows][n_par], the evaluator's value of each leaf's state: the return it expects
 *            from that state to the end of the episode.  leaf_prior_dev: NULL, or fp32 [rows][n_par][k_cap], weights per net for the
 *            children of each lane's leaf.
 *   Return.  Per row, in lane order: G = the line's return for a TERMINAL leaf (its value entry is not read); otherwise G = ret + v, one
 *            IEEE addition, v the lane's value entry, or 0.0 where that entry is not finite.
 *   Backup.  v1's Backup rule: on every node of the path N += 1, V -= 1, W += G; then min = fmin(min, G), max = fmax(max, G).
 *   Best line.  From TERMINAL simulations only (only there is G an exact episode return): if G > best (strictly: the first wins) best = G
 *            and the best order becomes the path.  A session without a terminal simulation has best return -inf and best order all 0.
 *   Leaf priors.  After the lane's backup, if leaf_prior_dev is given and the lane's leaf is FRESH: the P of its children block is
 *            overwritten by v1's Prior rule from that lane's row — S summed in double over the block's nets in ascending net order,
 *            entries that are not finite or are < 0 count as 0, P = w[net] / S; S == 0 leaves the block as it is.  A leaf that is not
 *            FRESH (terminal, unexpanded, or expanded by an earlier wave) is never given a new prior.
 *   Outputs. Every backup writes visits_out_dev (int32 [rows][k_cap]) and value_out_dev (double [rows][k_cap]) of the root's children
 *            as v1 does, info_out_dev int32 [rows][4] = {simulations so far, nodes_used, max_depth, flags (XR_TREE_POOL_FULL)}, and,
 *            where given, best_order_out_dev (int32 [rows][k_cap]), best_return_out_dev (double [rows]) and returns_out_dev (double
 *            [rows][n_par], the wave's G; 0.0 for a done row): the caller may stop after any wave.
 * Call order.  XR_ERR_STATE for xr_batch_tree_leaves before a successful open of that pool, or twice without a backup between; for
 * xr_batch_tree_backup without pending leaves; for any of the three where the kernels are not linked.  XR_ERR_RANGE for a wave that
 * would pass max_sims (the tree is unchanged).  After xr_batch_set_groups or xr_batch_load_regions the caller must re-open.
 * Errors (the batch and the session are untouched after any of them): XR_ERR_INVALID null b, a group outside -1 .. n_groups - 1, a c_init
 * that is not finite, a c_base that is not > 0 and finite (open); null rows_out_dev / out_dev, rows_out_dev not 8-byte aligned or
 * row_bytes % 8 != 0 (leaves); null value_dev / visits_out_dev / value_out_dev / info_out_dev (backup); XR_ERR_STATE before
 * xr_batch_load_regions; XR_ERR_RANGE n_par outside 1 .. XR_PEEK_MAX, max_sims outside n_par .. XR_TREE_MAX_SIMS, node_cap < 1,
 * k_cap < k_max, rows x n_par beyond 31 bits (open), row_bytes < xr_batch_state_row_bytes (leaves), and for the HBM-scratch router forms
 * (force_scratch_field included) and stream_per_region, for the rollout's reason; XR_ERR_NOMEM when the pool cannot be allocated.  Every
 * message names the entry point.
 * Contract, v1's and peek's.  None of the three ever synchronises: each only enqueues on `stream` (open: the table's copy and one launch;
 * leaves: select and the persistent peek launch; backup: one launch; no workgroup waits for another one).  They leave NO TRACE in the
 * batch: the peek launch plays in lookahead's shadow slots, every array xr_batch_fetch returns is only read, and the validity of the
 * in-place observation buffers is kept.  Sessions of DIFFERENT groups may be in flight at once on different streams; within one group
 * (or for the whole batch) the calls of a session, other searches, peeks, rollouts, lookaheads, branches and steps are ordered by the
 * caller, and so is the evaluator: it runs on `stream`, or is ordered against it by the caller.
 * A session started by xr_batch_tree_open is not keyed (see xr_batch_tree_reopen below): the next reopen rebuilds every row.
 * Cuts: no Dirichlet noise, no discounting, no HBM-scratch forms; no kept tree for this form in a session started by
 * xr_batch_tree_open (it starts from an empty tree): the kept tree is xr_batch_tree_reopen's ("XR-Tree v2, kept", below). */
#define XR_TREE_LEAF_TERMINAL 1
#define XR_TREE_LEAF_FRESH 2
#define XR_TREE_LEAF_NONE 4
int32_t xr_batch_tree_open(xr_batch* b, int32_t group, int32_t n_par, int32_t node_cap, double c_init, double c_base,
                           int32_t max_sims, const float* root_prior_dev, int32_t k_cap, void* stream);
int32_t xr_batch_tree_leaves(xr_batch* b, int32_t group, uint8_t* rows_out_dev, int64_t row_bytes, int32_t region_base,
                             int32_t* out_dev, double* return_out_dev, int32_t* paths_out_dev, int32_t* leaf_out_dev, void* stream);
int32_t xr_batch_tree_backup(xr_batch* b, int32_t group, const double* value_dev, const float* leaf_prior_dev,
                             int32_t* visits_out_dev, double* value_out_dev, int32_t* info_out_dev,
                             int32_t* best_order_out_dev, double* best_return_out_dev, double* returns_out_dev, void* stream);

/* ---- kept evaluated trees: a session that continues after a real step ---- */
/* xr_batch_tree_reopen is xr_batch_tree_open in every argument the two share: the same checks in the same order and the same error
 * codes (every message names xr_batch_tree_reopen), the same refusal of the HBM-scratch forms and of stream_per_region, the
 * enqueue-only contract and the no-trace contract, the same caller's evaluated-tree pool.  It ends the pool's last session and starts
 * a new one; xr_batch_tree_leaves and xr_batch_tree_backup then run on that session unchanged.  What differs is where the new session's
 * trees come from: the subtree below the net the env has really played since the last session.  "XR-Tree v2, kept" — "XR-Tree v1, kept"
 * (the kept trees section above) carried over to this pool:
 *   Key.     A session started by reopen is KEYED: its first kernel ends by writing, per row, the env's env_steps, region, replay and a
 *            valid bit.  The session's snapshot of the legal words is the key's legal words: there is no second copy.  A session started
 *            by xr_batch_tree_open is not keyed.
 *   Host-side rebuild of every row.  The kernel receives played == NULL when played_dev is NULL (a fresh session that leaves a keyed
 *            tree behind); when the pool's last session was not keyed; when that session still has leaves waiting for a backup (pending
 *            visits V are in its nodes); when rows, the group's first slot, node_cap, k_cap, legal_words or n_par differ from that
 *            session's; and when the pool had to be allocated again.  max_sims, c_init, c_base and the prior may differ.  After
 *            xr_batch_set_groups or xr_batch_load_regions every row is rebuilt.
 *   played_dev.  Otherwise int32 [rows], a = played[row]:
 *            a == 0: the row is kept whole if the key is valid, equals the env's current env_steps, region, replay and legal words
 *            exactly, and the kept root's N + max_sims <= XR_TREE_MAX_SIMS.
 *            a > 0: the row is re-rooted if all of these hold: the key is valid; region and replay are equal; env_steps ==
 *            key.env_steps + 1; bit a is set in the key's legal words; the env's legal words equal the key's with bit a cleared; the kept
 *            root is expanded and has a child of net a; that child's N + max_sims <= XR_TREE_MAX_SIMS.
 *            Otherwise, and for any negative entry, the row is rebuilt exactly as xr_batch_tree_open builds it.  A rebuild is never an
 *            error.
 *   Re-rooting (normative, node numbering included).  New node 0 is the old child of a, with net = 0 and P = 1.0.  The new nodes are
 *            then taken in index order, and the children block of every expanded one is appended in its old (ascending net) order: a
 *            breadth-first compaction.  Let r be the slot's reward row (the reward of the step that played a).  Every copied node gets
 *            W' = W - (double)N * r: one multiplication, then one subtraction, each rounded on its own, contraction off; N, P, net and
 *            count are kept, V is 0.  The row state gets min' = min - r and max' = max - r (infinities stay).  With a == 0 nothing is
 *            shifted or renumbered.  In both cases best restarts at -inf and the pool's best order at all 0, max_depth restarts at 0, the
 *            flags become XR_TREE_KEPT alone, the snapshot (nlegal, legal words) becomes the env's current one, and the pool's row prior
 *            becomes this call's root_prior_dev (uniform when NULL): it serves the new expansions of this session.  Kept nodes keep the
 *            P they have, a P an evaluator's leaf prior gave them included.  A new root that is unexpanded is expanded at once under this
 *            call's prior.  A carried node is never FRESH again, so a leaf prior never overwrites its block.  A row whose env has no
 *            legal net is a done row: v1's empty result, kept {0, 0}.
 *   Table and counting.  A reopen session indexes E[0 .. XR_TREE_MAX_SIMS], the kept search's formula, uploaded once per (c_init,
 *            c_base): Select never clamps at a carried root.  The session's simulation counter starts at 0: max_sims bounds THIS
 *            session's simulations, xr_batch_tree_leaves refuses the wave that would pass it, and info[0] is this session's
 *            simulations.  visits_out / value_out show the root's children with the carried visits included, in the current frame.
 *   kept_out_dev.  NULL, or int32 [rows][2] = {N of the new root before this session's simulations, nodes carried}; {0, 0} for a
 *            rebuilt row.
 *   Memory.  The pool of a keyed session holds two halves of rows x node_cap nodes (a reopen re-roots from the half the last session
 *            searched in into the other one) and a key per row beside what a plain session holds:
 *            rows x (80 node_cap + 40 + n_par x (4 k_cap + 16) + 8 k_cap + 8 legal_words + 4 + 24) bytes, each of its eleven arrays (the
 *            two halves, row states, paths, line returns, leaf records, best order, legal words, nlegal, prior, keys) rounded up to 16,
 *            allocated again when a call needs more than any before it, plus 8 x (XR_TREE_MAX_SIMS + 1) bytes per distinct (c_init,
 *            c_base) for the table.  xr_batch_tree_open keeps its own formula and carve of the same allocation.  A reopen that has to
 *            allocate has nothing to keep and rebuilds every row.
 * Cuts: the best line does not carry (best_order and best_return are this session's terminal simulations' alone); at most one real
 * route between two sessions (a row whose env made two is rebuilt); a tree does not follow xr_batch_branch to another slot; an abandoned
 * wave (leaves without backup) forfeits the tree. */
int32_t xr_batch_tree_reopen(xr_batch* b, int32_t group, const int32_t* played_dev,
                             int32_t n_par, int32_t node_cap, double c_init, double c_base, int32_t max_sims,
                             const float* root_prior_dev, int32_t k_cap, int32_t* kept_out_dev, void* stream);

/* ---- XR-Maze v2: global-route guides (optional) ---------------------------------------------- */
/* The reference's simulator runs with `-follow_guide 1` (ispd/ispd18_test1/run-net-ordering-training.tcl:3) on the guide file
 * it ships (ispd/ispd18_test1/ispd18_test1.input.guide: per net, rectangles per metal layer).  With xr_config.guide_cost > 0 a
 * net's guide is, by default, the bounding box of its access points; this call replaces it, per (region, net), by up to
 * XR_GUIDE_MAX_BOXES boxes (x0, y0, x1, y1, z0, z1: track / layer indices of the region's grid, inclusive — the guide
 * rectangles clipped to the region, xroute_env_amd/lefdef.py): a node is inside the guide when it lies in any box inflated by
 * guide_margin tracks in x and y.  box_off_host[r] = int32[n_nets(r) + 1] offsets (0-based nets) into boxes_host[r] =
 * int16[boxes][6]; box_off_host[r] == NULL: region r keeps the default guides; box_off_host == NULL: drop every guide.
 * A net with no box keeps the default guide.  Call after xr_batch_load_regions (a reload drops the guides); host pointers,
 * copied before the call returns.  Build-defined like the rest of XR-Maze (parity unpinned against the reference's router). */
#define XR_GUIDE_MAX_BOXES 8
int32_t xr_batch_load_guides(xr_batch* b, const int32_t* const* box_off_host, const int16_t* const* boxes_host, void* stream);

/* ---- stateless observation build --------------------------------------------------------- */
/* Replaces build_3Dgrid(data, routed_nets, bool_inference) for a caller that already holds the
 * node records (the inference servers baseline/DQN/test_DQN.py:54-62, baseline/PPO/test_PPO.py:
 * 58-62): nets_dev = the K legal 1-based net ids in ascending order. out_dev: (2+7K)*N floats. */
int32_t xr_observation_from_records(const uint32_t* nodes_dev, int32_t dim_x, int32_t dim_y,
                                    int32_t dim_z, const int32_t* nets_dev, int32_t k,
                                    float* out_dev, void* stream);

/* ---- agent side (a consumer of the path) ----------------------------------- */
/* The obstacle tower of the reference's RepresentationNetwork (baseline/baseline_utils.py:231-379: ob_conv1 -> ob_align_conv1 ->
 * ob_conv2 -> ob_align_conv2, what its DQN / PPO agents run on plane 0 of every observation before choosing a net) as one fused
 * kernel, eval mode: head_dev fp32 [n_envs][head_stride] with plane 0 of every env first (the buffers of xr_batch_step_compact /
 * xr_batch_step_observe), (D, H, W) = the observation tensor's trailing dims (dim_z, dim_y, dim_x), weights_dev =
 * xr_agent_obstacle_tower_weights() floats packed by xroute_env_amd/agents.py FusedObstacleTower.refresh (BatchNorm folded; the two 7 -> 7-channel
 * convolutions as the per-lane A operands of the kernel's v_mfma_f32_16x16x4_f32 steps: csrc/xr_agent.hip XT_* offsets), out_dev fp32 [n_envs][64]
 * (normalize != 0: after the reference's row-wise min-max normalisation, baseline/baseline_utils.py:45-63).  XR_ERR_RANGE: a grid shape the kernel does not take (use the framework path). */
int32_t xr_agent_obstacle_tower_weights(void);
int32_t xr_agent_obstacle_tower(const float* head_dev, int64_t head_stride, int32_t n_envs, int32_t dim_d, int32_t dim_h, int32_t dim_w,
                                const float* weights_dev, float* out_dev, int32_t normalize, void* stream);
/* The actor head (baseline/DQN/DQN.py:27-46 `Actor`: mlp 128 -> 128 -> 64 -> 1, ELU, on [state vector ++ net vector]) for every legal net of
 * every env + the greedy action (DQN.inference_action; PPO samples from the same logits): state_dev fp32 [n_envs][64] normalised state
 * vectors, the net ids from the net-order channel of head_dev (plane 1, `ids_off` floats into an env's row), the normalised net vectors from
 * cache_vec_dev [regions * cache_kmax][64] (row = region * cache_kmax + net - 1: agents.NetVectorCache, complete) or, when cache_pre_dev
 * [regions * cache_kmax][128] is given, from the first layer's net half already applied to them (W1[:, 64:] . vec, once per weight update), weights_dev =
 * xr_agent_actor_weights() floats (transposed by agents.FusedActorHead).  logits_dev: optional fp32 [n_envs][kcap], -inf beyond an env's
 * nets; action_dev int32 [n_envs]: first maximum in the channel's order, 0 without nets.  An env with nlegal <= 0 (a row that xr_batch_expand_state
 * flagged with nlegal = region = -1 included) gets action 0 and a logits row of -inf.  With cache_pre_dev kcap is at most 256 (XR_ERR_RANGE beyond);
 * with cache_pre_dev == NULL any kcap is taken. */
int32_t xr_agent_actor_weights(void);
int32_t xr_agent_actor(const float* state_dev, const float* head_dev, int64_t head_stride, int32_t ids_off, const int32_t* nlegal_dev,
                       const int32_t* region_dev, const float* cache_vec_dev, const float* cache_pre_dev, int32_t cache_kmax, const float* weights_dev,
                       int32_t n_envs, int32_t kcap, float* logits_dev, int32_t* action_dev, void* stream);
/* ABI 8: the same kernel with PPO's rollout sampling inside (baseline/PPO/PPO.py:124-146 `ActorCritic.act`: `dist = Categorical(action_probs); action =
 * dist.sample()`; caller `select_action`, :205-217).  env_ids_dev int64 [n_envs] = the GLOBAL id of every env, s0 = the (seed, step) word of
 * xroute_env_amd.agents.counter_uniform: action_dev = a sample of Categorical(softmax(logits)) by the Gumbel-max trick over counter-based uniforms of
 * (s0, global env id, rank of the net) — no generator state, so an env gets the same action whichever rank or batch evaluates it, and the same one the
 * framework path's tensor ops choose (same integer hash, same float operations in the same order).  env_ids_dev == NULL: the greedy action. */
int32_t xr_agent_actor_sample(const float* state_dev, const float* head_dev, int64_t head_stride, int32_t ids_off, const int32_t* nlegal_dev,
                              const int32_t* region_dev, const float* cache_vec_dev, const float* cache_pre_dev, int32_t cache_kmax, const float* weights_dev,
                              int32_t n_envs, int32_t kcap, float* logits_dev, int32_t* action_dev, const int64_t* env_ids_dev, uint64_t s0, void* stream);

/* The NET tower of the same network (ABI 9: `net_conv1 -> net_align_conv1 -> net_conv2 -> net_align_conv2`, baseline/baseline_utils.py:246-262, 350-357) for
 * n_pairs (region, net) pairs of ONE grid shape (D, H, W) = (dim_z, dim_y, dim_x), straight from the access-point lists of the regions loaded in `b` — the 7 planes
 * of a net (baseline/build_3Dgrid.py:106-142) are never formed: they are 0/1 planes whose non-zeros are the net's access points, ResidualBlock(7) of such an input
 * differs from its response to an empty grid only within two voxels of one, and the aligning convolution is linear (xr_agent.hip, the NET branch).
 *   pair_region_dev / pair_net_dev  int32 [n_pairs]: region index in `b`, 1-based net id
 *   weights_dev   xr_agent_net_tower_weights() floats, bg_dev fp32 [od*oh*ow*7] = align1(block(0)) of this shape: both packed by agents.FusedNetTower
 *   out_dev       fp32 [n_pairs][64] (min-max normalised when normalize != 0, like the obstacle tower's rows)
 *   flags_dev     int32 [n_pairs], ZEROED BY THE CALLER: 1 = the net's neighbourhood lists do not fit LDS (more than ~20 scattered access points: the caller's
 *                 framework path takes that net), 2 = the pair names a region of another shape or a net it does not have; such rows of out_dev stay unwritten
 * XR_ERR_RANGE for grid shapes the kernel does not take. */
int32_t xr_agent_net_tower_weights(void);
/* How the towers' 7 -> 7-channel convolutions run (both kernels): 1 (default) = split-bf16 operands on v_mfma_f32_16x16x32_bf16 — every fp32 weight and activation held
 * as hi = bf16(v), lo = bf16(v - hi), a product as hi x hi + hi x lo + lo x hi accumulated in fp32 (normalised vectors within 1.1e-5 of the fp32 form on the reference
 * fixtures); 0 = fp32 operands on v_mfma_f32_16x16x4_f32 (environment XR_TOWER_FP32=1 before the first call).  Both weight layouts travel in the packed vectors. */
int32_t xr_agent_matrix_mode(void);
int32_t xr_batch_net_vectors(xr_batch* b, const int32_t* pair_region_dev, const int32_t* pair_net_dev, int32_t n_pairs, int32_t D, int32_t H, int32_t W,
                             const float* weights_dev, const float* bg_dev, float* out_dev, int32_t* flags_dev, int32_t normalize, void* stream);

/* ---- wire format (net_ordering.proto v1), host only ---------------------------------------- */
/* Replaces handle_messange's protobuf decode (baseline/baseline_utils.py:9-43; the `message.ParseFromString` of :418,467), with the
 * runtime's parse rules: the oneof keeps the LAST member on the wire, a repeated occurrence of the same member merges (scalars: last
 * value, `nodes` / `nets`: appended), unknown fields of every wire type (groups included) are skipped, packed and unpacked `nets` mix.
 * Pass 1 (fields_host == NULL, nets_host == NULL): fills info_host[8] = {kind (1 request, 2 response, 0 empty),
 * dim_x, dim_y, dim_z, n_nodes, n_nets, is_done, response.net_index} and metrics_host[3].
 * Pass 2: fields_host int32[fields_cap][10] = maze xyz, point xyz, type, is_used, net, pin (wire values, 0-based);
 * nets_host uint32[nets_cap].  Capacities are in rows / entries; nothing is ever written past them (ABI 9: round 5's two-pointer form
 * trusted pass 1's counts, which a oneof flip makes smaller than what an earlier, dropped member held).  XR_ERR_RANGE when what the
 * message finally holds does not fit (info_host carries the counts needed); XR_ERR_PARSE for bytes the runtimes refuse. */
int32_t xr_proto_decode(const uint8_t* buf_host, size_t len, int64_t* info_host, uint32_t* metrics_host,
                        int32_t* fields_host, int64_t fields_cap, uint32_t* nets_host, int64_t nets_cap);
/* Encodes Message{response{net_index}} exactly as Game.step does (:409-411). Returns bytes written
 * through *len (buf capacity >= 16). */
int32_t xr_proto_encode_response(int32_t net_index, uint8_t* buf_host, size_t* len);
/* Encodes Message{request{...}} (the simulator side; used by tests and the serve-the-protocol path).
 * Call with buf_host == NULL to get the required size in *len. */
int32_t xr_proto_encode_request(int32_t dim_x, int32_t dim_y, int32_t dim_z, const int32_t* fields_host,
                                int32_t n_nodes, const uint32_t* metrics_host, int32_t is_done,
                                const uint32_t* nets_host, int32_t n_nets, uint8_t* buf_host, size_t* len);

#ifdef __cplusplus
}
#endif
#endif /* XROUTE_HIP_H */
