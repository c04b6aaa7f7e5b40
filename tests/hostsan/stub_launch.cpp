// tests/hostsan/stub_launch.cpp — TEST INFRASTRUCTURE (see hip/hip_runtime.h of this directory): the kernel launchers xr_device.h
// declares, doing nothing.  Everything the sanitizer build exercises happens BEFORE a launch: validation, staging, copies, bookkeeping.
#include <hip/hip_runtime.h>

#include "../../xroute_env_amd/csrc/xr_device.h"

extern "C" {
int64_t xr_stub_alloc_limit = -1;
int64_t xr_stub_alloc_live = 0;
int64_t xr_stub_launches = 0;
// optional (null: off, what the Python drivers leave it at): called by every launcher with its name, the batch view and the router
// variant it was handed (null where the launcher takes none) — load_trace.cpp prints what reaches a launch through it
void (*xr_stub_launch_hook)(const char* name, const XrBatchDev* b, const XrRouteVariant* v) = nullptr;
void (*xr_stub_malloc_hook)(size_t bytes) = nullptr;      // optional: the byte count of every hipMalloc (hip/hip_runtime.h)
void (*xr_stub_alloc_hook)(void* p, size_t bytes, int freed) = nullptr;                                   // optional, both: hip/hip_runtime.h
void (*xr_stub_async_hook)(const char* what, const void* dst, int kind, size_t bytes) = nullptr;
}

static hipError_t launched(const char* name, const XrBatchDev* b = nullptr, const XrRouteVariant* v = nullptr) {
    xr_stub_launches++;
    if (xr_stub_launch_hook) xr_stub_launch_hook(name, b, v);
    return hipSuccess;
}

extern "C" {
hipError_t xr_launch_ingest(const uint32_t*, int16_t*, int16_t*, int64_t, hipStream_t) { return launched("ingest"); }
hipError_t xr_launch_reset(const XrBatchDev* b, const uint8_t*, int, hipStream_t) { return launched("reset", b); }
hipError_t xr_route_set_max_lds(size_t) { return hipSuccess; }
hipError_t xr_launch_route(const XrBatchDev* b, const int32_t*, XrRouteVariant v, hipStream_t) { return launched("route", b, &v); }
hipError_t xr_route_occupancy(XrRouteVariant, int* per_cu, size_t* lds) { if (per_cu) *per_cu = 1; if (lds) *lds = 0; return hipSuccess; }
hipError_t xr_launch_plan(const XrBatchDev* b, const int32_t*, uint32_t*, int32_t*, int*, hipStream_t) { return launched("plan", b); }
hipError_t xr_launch_route_order(const XrBatchDev* b, const int32_t*, int32_t*, hipStream_t) { return launched("route_order", b); }
hipError_t xr_launch_step_queue(const XrBatchDev* b, const int32_t*, XrRouteVariant v, int, hipStream_t) { return launched("step_queue", b, &v); }
hipError_t xr_launch_netplanes(const XrBatchDev* b, int, int, hipStream_t) { return launched("netplanes", b); }
hipError_t xr_launch_order(const XrBatchDev* b, const int32_t*, int, int32_t*, XrRouteVariant v, hipStream_t) { return launched("order", b, &v); }
hipError_t xr_launch_random_actions(const XrBatchDev* b, int32_t*, uint64_t, hipStream_t) { return launched("random_actions", b); }
hipError_t xr_launch_obs(const XrBatchDev* b, float*, int64_t, int, int, int, int, hipStream_t) { return launched("obs", b); }
hipError_t xr_launch_obs_u8(const XrBatchDev* b, uint8_t*, int64_t, int, int, int, int, hipStream_t) { return launched("obs_u8", b); }
hipError_t xr_launch_obs_records(const uint32_t*, int, int, int, const int32_t*, int, float*, int, hipStream_t) { return launched("obs_records"); }
hipError_t xr_launch_unit_helpers(const XrBatchDev* b, int, hipStream_t) { return launched("unit_helpers", b); }
hipError_t xr_launch_netplanes_pairs(const XrBatchDev* b, const int32_t*, const int32_t*, int, float*, int64_t, int, hipStream_t) { return launched("netplanes_pairs", b); }
hipError_t xr_launch_pack_state(const XrBatchDev* b, uint8_t*, int64_t, int, hipStream_t) { return launched("pack_state", b); }
hipError_t xr_launch_guide_masks(const XrBatchDev* b, uint8_t*, int, hipStream_t) { return launched("guide_masks", b); }
hipError_t xr_launch_ingest_state(const XrBatchDev* b, const int16_t*, const uint64_t*, const int32_t*, hipStream_t) { return launched("ingest_state", b); }
hipError_t xr_launch_net_tower(const void*, const int32_t*, const int32_t*, int32_t, const int32_t*, const int32_t*, int32_t, int32_t, int32_t, int32_t, const float*, const float*,
                               float*, int32_t*, int32_t, hipStream_t, int32_t* status) { *status = 0; return launched("net_tower"); }
hipError_t xr_launch_expand_state(const XrBatchDev* b, const uint8_t*, int64_t, int, float*, int64_t, int32_t*, int32_t*, int, hipStream_t) { return launched("expand_state", b); }
}
