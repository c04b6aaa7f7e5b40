// tests/hostsan/stub_launch_search.h — TEST INFRASTRUCTURE (see hip/hip_runtime.h of this directory): what the search launchers of
// stub_launch_search.cpp hand to their hook, one record per argument, in the launcher's argument order.
#pragma once
#include <cstdint>

struct XrStubArg {
    const char* name;
    char kind;            // 'i' signed, 'u' unsigned (printed in hex: seeds), 'f' double, 'p' pointer
    int64_t i;
    uint64_t u;
    double f;
    const void* p;
};
// optional (null: off): called by every search launcher with its name and its arguments
extern "C" void (*xr_stub_search_hook)(const char* launcher, const XrStubArg* args, int n);
