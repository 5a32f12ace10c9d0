// Stand-alone host check of the persistent decode's hand-off arena (nanollama_amd/csrc/nl_persist.h: pd_arena).
// Built and run on the CPU by tests/test_persist_arena.py, once plain and once under the address / undefined-behaviour sanitizers.
// For both instantiated shape classes (D 576 / I 1536 / H 9, D 256 / I 512 / H 4), their kv-head counts and L = 1 .. 16 it walks
// every granule a phase of pd_decode_kernel stores or polls -- with the kernel's own arithmetic: scalar offset (area + record) plus
// lane offset -- into a byte map of the arena:
//   1. every area starts on a 16-byte boundary, every access is aligned to its width;
//   2. no byte belongs to two areas (or to the same area of two layers);
//   3. every access ends inside the total of the model's L (and so inside the kernel's buffer resource: the arena of PD_MAXL layers,
//      which is what the host allocates);
//   4. the areas written from other XCDs (am; x of every record) are whole 128-byte lines, and tok has a line of its own;
//   5. the area offsets and the record stride do not depend on L (the kernel takes them from pd_arena(D, I, H, PD_MAXL), the host
//      allocates that form's total), and the total is far below 2^31.
#include <algorithm>
#include <cstdio>
#include <vector>
#include "nl_persist.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails < 50) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } fails++; } } while (0)

enum { A_TOK = 1, A_AM, A_X, A_QKV, A_O, A_XP, A_H, A_PART };

struct Map {
    std::vector<int> owner;      // per byte: 0 = unused, else area * 64 + layer + 1
    nl::PdArena A;
    int D, I, H, KV, L;
    unsigned long long hi = 0;   // largest end of an access
    void touch(int area, int layer, unsigned long long soff, unsigned long long voff, unsigned width, const char *what) {
        const unsigned long long at = soff + voff;
        CHECK(at % width == 0, "D %d KV %d L %d %s layer %d: offset %llu is not aligned to %u", D, KV, L, what, layer, at, width);
        CHECK(at + width <= nl::pd_arena(D, I, H, nl::PD_MAXL).total, "D %d KV %d L %d %s layer %d: %llu + %u beyond the range of the kernel's resource", D, KV, L, what, layer, at, width);
        CHECK(at + width <= A.total, "D %d KV %d L %d %s layer %d: %llu + %u beyond the total %u", D, KV, L, what, layer, at, width, A.total);
        if (at + width > A.total) return;
        hi = std::max(hi, at + width);
        const int key = area * 64 + layer + 1;
        for (unsigned b = 0; b < width; b++) {
            int &o = owner[at + b];
            CHECK(o == 0 || o == key, "D %d KV %d L %d %s layer %d: byte %llu also belongs to area %d of layer %d", D, KV, L, what, layer, at + b, o / 64, o % 64 - 1);
            o = key;
        }
    }
};

static void check(int D, int I, int H, int KV, int L) {
    using namespace nl;
    Map M;
    M.A = pd_arena(D, I, H, L); M.D = D; M.I = I; M.H = H; M.KV = KV; M.L = L;
    const PdArena A = M.A, A0 = pd_arena(D, I, H, 0);
    // 5. the offsets are the same for every L (compared against the L = 0 form)
    CHECK(A.tok == A0.tok && A.am == A0.am && A.layers == A0.layers && A.x == A0.x && A.qkv == A0.qkv && A.o == A0.o && A.xp == A0.xp && A.h == A0.h &&
          A.part == A0.part && A.layer_stride == A0.layer_stride, "D %d L %d: an offset depends on L", D, L);
    CHECK((unsigned long long)A0.layers + (unsigned long long)(L + 1) * A0.layer_stride == A.total && A.total < (1u << 24), "D %d L %d: total %u", D, L, A.total);
    // 1. / 4. area starts
    const unsigned starts[] = {A.tok, A.am, A.layers, A.x, A.qkv, A.o, A.xp, A.h, A.part, A.layer_stride, A.total};
    for (unsigned s : starts) CHECK(s % 16 == 0, "D %d L %d: area start / size %u is not a multiple of 16", D, L, s);
    CHECK(A.am % 128 == 0 && A.am >= 128 && A.tok + 8 <= 128 && (PD_GRID * 16) % 128 == 0, "D %d: am / tok lines", D);
    CHECK(A.layers % 128 == 0 && A.layer_stride % 128 == 0 && A.x % 128 == 0 && (A.qkv - A.x) % 128 == 0 && A.qkv - A.x == (unsigned)D * 8u, "D %d: x is not whole lines", D);
    M.owner.assign(A.total, 0);
    const int KVD = KV * 64, GQ = H / KV, QR = (D + 2 * KVD) / PD_CUS, WR = D / PD_CUS;
    const int VPG = pd_h_vpg(I), HS = I / VPG, HSU = HS / PD_CUS;
    auto area = [&](unsigned a, int layer) { return (unsigned long long)A0.layers + a + (unsigned long long)layer * A0.layer_stride; };     // PD_AREA
    // the doorman's token word; the 256 argmax granules (store: cu * 16, poll: tid * 16)
    M.touch(A_TOK, 0, A.tok, 0, 8, "tok");
    for (int cu = 0; cu < PD_GRID; cu++) M.touch(A_AM, 0, A.am, (unsigned)cu * 16u, 16, "am");
    for (int layer = 0; layer <= L; layer++) {
        // x: gathered by every thread (pd_gather<2>: granule min(tid + 512 k, D - 1)), published per row of the layer before (idx * WR + row)
        for (int tid = 0; tid < PD_THREADS; tid++)
            for (int k = 0; k < 2; k++) M.touch(A_X, layer, area(A0.x, layer), (unsigned)std::min(tid + k * PD_THREADS, D - 1) * 8u, 8, "x gather");
        for (int idx = 0; idx < PD_CUS; idx++)
            for (int row = 0; row < WR; row++) M.touch(A_X, layer, area(A0.x, layer), (unsigned)(idx * WR + row) * 8u, 8, "x publish");
        if (layer == L) break;       // record L holds only x
        // q | k | v rows per unit; the heads' polls
        for (int idx = 0; idx < PD_CUS; idx++)
            for (int r = 0; r < QR; r++) M.touch(A_QKV, layer, area(A0.qkv, layer), (unsigned)(idx * QR + r) * 8u, 8, "qkv publish");
        for (int hidx = 0; hidx < H; hidx++)
            for (int tid = 0; tid < 192; tid++) {
                const int sect = tid >> 6, e = tid & 63;
                const unsigned off = (unsigned)((sect == 0 ? hidx * 64 : sect == 1 ? D + (hidx / GQ) * 64 : D + KVD + (hidx / GQ) * 64) + e) * 8u;
                CHECK(off / 8 < (unsigned)(D + 2 * KVD), "D %d KV %d: head %d polls q|k|v granule %u of %d", D, KV, hidx, off / 8, D + 2 * KVD);
                M.touch(A_QKV, layer, area(A0.qkv, layer), off, 8, "qkv poll");
            }
        // o per head (publish lane / tid < 64; gather as x)
        for (int hidx = 0; hidx < H; hidx++)
            for (int l = 0; l < 64; l++) M.touch(A_O, layer, area(A0.o, layer), (unsigned)(hidx * 64 + l) * 8u, 8, "o publish");
        for (int tid = 0; tid < PD_THREADS; tid++)
            for (int k = 0; k < 2; k++) M.touch(A_O, layer, area(A0.o, layer), (unsigned)std::min(tid + k * PD_THREADS, D - 1) * 8u, 8, "o gather");
        // x'
        for (int idx = 0; idx < PD_CUS; idx++)
            for (int row = 0; row < WR; row++) M.touch(A_XP, layer, area(A0.xp, layer), (unsigned)(idx * WR + row) * 8u, 8, "x' publish");
        for (int tid = 0; tid < PD_THREADS; tid++)
            for (int k = 0; k < 2; k++) M.touch(A_XP, layer, area(A0.xp, layer), (unsigned)std::min(tid + k * PD_THREADS, D - 1) * 8u, 8, "x' gather");
        // h: unit idx publishes granule idx * HSU + i, whose values are its local rows k * HSU + i = h rows g + k S (pd_h_row); lane tid polls granule tid
        for (int idx = 0; idx < PD_CUS; idx++)
            for (int i = 0; i < HSU; i++) {
                const int g = idx * HSU + i;
                for (int k = 0; k < VPG; k++) CHECK(pd_h_row(idx, k * HSU + i, I) == g + k * HS, "I %d: unit %d granule %d value %d is h row %d", I, idx, g, k, pd_h_row(idx, k * HSU + i, I));
                M.touch(A_H, layer, area(A0.h, layer), (unsigned)g * 16u, 16, "h publish");
            }
        for (int tid = 0; tid < PD_THREADS; tid++)
            if ((tid >> 6) * 64 < HS) M.touch(A_H, layer, area(A0.h, layer), (unsigned)std::min(tid, HS - 1) * 16u, 16, "h gather");
        // the helpers' records: part p of head hidx publishes record (hidx * (PD_PARTS - 1) + p - 1); the owner polls its PD_PARTS - 1 records
        for (int hidx = 0; hidx < H; hidx++) {
            for (int p = 1; p < PD_PARTS; p++) {
                const unsigned long long dst = area(A0.part, layer) + (unsigned long long)(hidx * (PD_PARTS - 1) + (p - 1)) * (66u * 8u);
                for (int tid = 0; tid < 64; tid++) M.touch(A_PART, layer, dst, (unsigned)(2 + tid) * 8u, 8, "part publish");
                M.touch(A_PART, layer, dst, 0, 8, "part publish M");
                M.touch(A_PART, layer, dst, 8, 8, "part publish L");
            }
            for (int tid = 0; tid < (PD_PARTS - 1) * 66; tid++)
                M.touch(A_PART, layer, area(A0.part, layer) + (unsigned long long)hidx * (unsigned)((PD_PARTS - 1) * 66 * 8), (unsigned)tid * 8u, 8, "part poll");
        }
    }
    CHECK(M.hi <= A.total, "D %d KV %d L %d: largest access ends at %llu, total %u", D, KV, L, M.hi, A.total);
    // 4. no line of a cross-XCD area holds anything else: the lines of tok, am and every x
    for (unsigned long long b = 0; b < A.total; b += 128) {
        int first = 0;
        bool mixed = false, cross = false;
        for (unsigned k = 0; k < 128 && b + k < A.total; k++) {
            const int o = M.owner[b + k];
            if (!o) continue;
            if (first && o != first) mixed = true;
            first = first ? first : o;
            cross = cross || o / 64 == A_AM || o / 64 == A_X || o / 64 == A_TOK;
        }
        CHECK(!(mixed && cross), "D %d KV %d L %d: the line at %llu mixes a cross-XCD area with another", D, KV, L, b);
    }
}

int main() {
    for (int L = 1; L <= nl::PD_MAXL; L++) {
        check(576, 1536, 9, 9, L);
        check(576, 1536, 9, 3, L);
        check(256, 512, 4, 4, L);
        check(256, 512, 4, 2, L);
    }
    CHECK(nl::pd_arena(576, 1536, 9, nl::PD_MAXL).total < (1u << 20), "the largest arena is %u bytes", nl::pd_arena(576, 1536, 9, nl::PD_MAXL).total);
    std::printf(fails ? "%d check(s) failed\n" : "pd_arena_check: ok\n", fails);
    return fails ? 1 : 0;
}
