// Stand-alone host check of the persistent decode's h granule layout (nanollama_amd/csrc/nl_persist.h: pd_h_vpg, pd_h_row).
// Built and run on the CPU by tests/test_persist_h_map.py, once plain and once under the address / undefined-behaviour sanitizers.
// For (I, VPG) = (1536, 3) and (512, 2):
//   1. (unit, local row) <-> h row is one to one;
//   2. the values of every granule g = {h[g], h[g + S], h[g + 2 S]} are rows of ONE unit, which publishes them as its granule
//      unit * (S / 32) + i from its local rows k * (S / 32) + i -- the kernel's publish;
//   3. consumer lane g holds elements g + k S: every half wavefront (32 lanes) holds, for each k, the 32 elements of one block in
//      lane order, and the blocks are covered once each.
#include <cstdio>
#include <vector>
#include "nl_persist.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); fails++; } } while (0)

static void check(int I, int want_vpg) {
    const int VPG = nl::pd_h_vpg(I);
    CHECK(VPG == want_vpg, "I %d: VPG %d, expected %d", I, VPG, want_vpg);
    if (VPG != want_vpg) return;
    const int S = I / VPG, SU = S / nl::PD_CUS, GR = I / nl::PD_CUS;
    CHECK(S * VPG == I && SU * nl::PD_CUS == S && GR == VPG * SU, "I %d: S %d, SU %d, GR %d", I, S, SU, GR);
    // 1. one to one
    std::vector<int> owner(I, -1), local(I, -1);
    for (int u = 0; u < nl::PD_CUS; u++)
        for (int lr = 0; lr < GR; lr++) {
            const int r = nl::pd_h_row(u, lr, I);
            CHECK(r >= 0 && r < I, "I %d: unit %d local row %d -> row %d out of range", I, u, lr, r);
            if (r < 0 || r >= I) continue;
            CHECK(owner[r] < 0, "I %d: row %d owned by units %d and %d", I, r, owner[r], u);
            owner[r] = u; local[r] = lr;
        }
    for (int r = 0; r < I; r++) CHECK(owner[r] >= 0, "I %d: row %d has no owner", I, r);
    // 2. a granule's values belong to one unit, and sit where that unit publishes them
    for (int g = 0; g < S; g++)
        for (int k = 0; k < VPG; k++) {
            const int r = g + k * S, u = owner[g], i = g - u * SU;
            CHECK(owner[r] == u, "I %d: granule %d value %d belongs to unit %d, value 0 to unit %d", I, g, k, owner[r], u);
            CHECK(i >= 0 && i < SU && local[r] == k * SU + i, "I %d: granule %d value %d is local row %d of unit %d, expected %d", I, g, k, local[r], u, k * SU + i);
        }
    // 3. whole blocks per half wavefront
    CHECK(S % 32 == 0, "I %d: S %d is not whole half wavefronts", I, S);
    std::vector<int> seen(I / 32, 0);
    for (int h = 0; h < S / 32; h++)
        for (int k = 0; k < VPG; k++) {
            const int blk = (h * 32 + k * S) >> 5;
            for (int l = 0; l < 32; l++) {
                const int e = h * 32 + l + k * S;
                CHECK((e >> 5) == blk && (e & 31) == l, "I %d: half wavefront %d value %d lane %d holds element %d, not lane %d of block %d", I, h, k, l, e, l, blk);
            }
            CHECK(blk == (h * 32 >> 5) + k * S / 32, "I %d: block %d", I, blk);
            seen[blk]++;
        }
    for (int b = 0; b < I / 32; b++) CHECK(seen[b] == 1, "I %d: block %d held by %d half wavefronts", I, b, seen[b]);
}

int main() {
    check(1536, 3);
    check(512, 2);
    CHECK(nl::pd_h_vpg(544) == 0 && !nl::pd_shape_ok(576, 1504, 9, 9, 64, 32000, 13), "a shape without a granule form must be refused");
    CHECK(nl::pd_shape_ok(576, 1536, 9, 9, 64, 32000, 13) && nl::pd_shape_ok(256, 512, 4, 2, 64, 1024, 5), "the two shapes of the kernel");
    std::printf(fails ? "%d check(s) failed\n" : "pd_h_map_check: ok\n", fails);
    return fails ? 1 : 0;
}
