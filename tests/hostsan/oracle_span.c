/* tests/hostsan/oracle_span.c — TEST INFRASTRUCTURE.  The CPU oracle (oracle/xr_oracle.c) under UBSan + ASan as a program of its own, on the
 * widest coordinates the loader's per-coordinate bounds admit: tracks at -2^30 and +2^30, a gap of 2^31 that no int32 difference holds.
 * tests/test_router_ranges_host.py builds it, runs it and compares the lines it prints; a sanitizer report ends it with a non-zero status. */
#include <stdio.h>

#include "../../oracle/xr_oracle.h"

#define REC_ACCESS(net1, pin1) (2u | ((uint32_t)(net1) << 3) | ((uint32_t)(pin1) << 17))

int main(void) {
    /* 4 x 3 x 2, layer 0 along x, layer 1 along y.  xs: two tracks at each end of [-2^30, 2^30]; ys likewise with one in the middle.
     * net 1: pins on the two tracks bordering the gap in x (unreachable: the edge is 2^31 - 800 >= XR_DIST_CAP);
     * net 2: pins 400 apart at the high end, on another row and layer (reached, one via). */
    const int X = 4, Y = 3, Z = 2;
    int32_t xs[4] = {-(1 << 30), -(1 << 30) + 400, (1 << 30) - 400, 1 << 30};
    int32_t ys[3] = {-(1 << 30), 0, 1 << 30};
    int32_t m0[3] = {0, 0, 0};
    uint8_t ldir[2] = {0, 1};
    uint32_t rec[4 * 3 * 2];
    for (int f = 0; f < X * Y * Z; f++) rec[f] = 1u;                      /* NORMAL */
#define F(x, y, z) (((x) * Y + (y)) * Z + (z))
    rec[F(1, 0, 0)] = REC_ACCESS(1, 1);
    rec[F(2, 0, 0)] = REC_ACCESS(1, 2);
    rec[F(2, 1, 0)] = REC_ACCESS(2, 1);
    rec[F(3, 1, 1)] = REC_ACCESS(2, 2);
    xro_env* e = xro_env_create(X, Y, Z, xs, ys, ldir, rec, 2, m0, 800, 8, 400);
    if (!e) return 2;
    uint32_t d[4 * 3 * 2];
    for (int net = 1; net <= 2; net++) {
        if (xro_env_distance_field(e, net, d)) return 3;
        printf("field %d:", net);
        for (int f = 0; f < X * Y * Z; f++) printf(" %u", d[f]);
        printf("\n");
    }
    for (int net = 1; net <= 2; net++) {
        int32_t delta[3], path[24];
        int done = 0, plen = 0;
        const int st = xro_env_step(e, net, delta, &done, path, 24, &plen);
        printf("step %d: status %d delta %d %d %d done %d path", net, st, delta[0], delta[1], delta[2], done);
        for (int i = 0; i < plen; i++) printf(" %d", path[i]);
        printf("\n");
    }
    xro_env_destroy(e);
    return 0;
}
