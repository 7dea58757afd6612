// Stand-alone check of the packed sweep grid (gibbssampler_amd/csrc/gs_sweep_pack.h),
// built and run by tests/test_sweep_pack_cpu.py with the host compiler.
//
// usage: sweep_pack_check L [L ...]
// For each L, with the rows per chunk the plan chooses, it walks the grid as the
// kernel does (cr_sweep_packed / cr_sweep_task in gs_kernels.hip) and checks:
//   * every (l, m), 0 <= m <= l <= L, lies in exactly one segment of exactly one
//     workgroup, plain workgroups included;
//   * a segment's rows are contiguous, ascending and inside one chunk, and one
//     thread runs it;
//   * every thread word decodes to an LDS slot (chunk, l-in-tile) in range, each
//     of the 256 slots of a packed workgroup is owned by exactly one thread, and
//     the wave's loop trips cover each of its threads' rows and are equal within
//     the wave;
//   * every (tile, chunk group) partial slot that the plain grid writes is written
//     by exactly one workgroup;
//   * with the option off the grid is the plain one.
// Prints one line per L: "L tm workgroups packed absorbed rows_plain rows_issued
// packed_m0 packed_partial": the last two count the packed workgroups that hold
// row m = 0 (chunk group 0) and those of a partial tile (lanes l < 0).
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "gs_sweep_pack.h"

using namespace gs_pack;

#define CHECK(c)                                                                          \
    do {                                                                                  \
        if (!(c)) {                                                                       \
            std::fprintf(stderr, "L %d: check failed at line %d: %s\n", L, __LINE__, #c); \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

static int check(int L) {
    const int tm = rows_per_chunk(L);
    const Plan P = build(L, tm, true);
    const Plan Q = build(L, tm, false);
    CHECK(P.ntile == (L + TILE) / TILE && P.nchunkg == (L / tm + 1 + CPG - 1) / CPG);
    CHECK((int)P.table.size() == P.ncls * NTHREAD);
    std::vector<int> seen((size_t)(L + 1) * (L + 1), 0);          // [m][l]
    std::set<std::pair<int, int>> slots;
    int npacked = 0, nabsorb = 0, npacked_m0 = 0, npacked_partial = 0;
    long long issued = 0;
    auto cover = [&](int l, int m0, int cnt, int chunk) {
        // rows m0 .. m0 + cnt - 1 of column l, all inside chunk `chunk`
        if (cnt <= 0) return true;
        if (l < 0 || l > L || m0 < 0 || m0 + cnt - 1 > l) return false;
        if (m0 / tm != chunk || (m0 + cnt - 1) / tm != chunk) return false;
        for (int m = m0; m < m0 + cnt; ++m) ++seen[(size_t)m * (L + 1) + l];
        return true;
    };
    for (const Group& g : P.groups) {
        const int lhi = L - TILE * g.tile;
        CHECK(g.tile >= 0 && g.tile < P.ntile && g.cg >= 0 && g.cg < P.nchunkg && lhi >= 0);
        CHECK(slots.insert({g.tile, g.cg}).second);
        issued += g.rows_issued;
        if (!g.packed) {
            // the plain form: wave w = chunk w, lane = l-in-tile, rows m0 .. min(m0 + tm, lhi + 1) - 1, m <= l
            CHECK(!g.absorb && g.rows_issued == g.rows_plain);
            for (int cq = 0; cq < CPG; ++cq)
                for (int lt = 0; lt < TILE; ++lt)
                    CHECK(cover(lhi - 63 + lt, (CPG * g.cg + cq) * tm, seg_rows(L, tm, g.tile, g.cg, cq, lt),
                                CPG * g.cg + cq));
            continue;
        }
        ++npacked;
        npacked_m0 += g.cg == 0 ? 1 : 0;
        npacked_partial += lhi < TILE - 1 ? 1 : 0;
        CHECK(g.cls >= 0 && g.cls < P.ncls);
        CHECK(g.absorb || g.rows_issued < g.rows_plain);
        CHECK(g.rows_issued <= g.rows_plain);
        const uint32_t* tab = P.table.data() + (size_t)g.cls * NTHREAD;
        bool slot_used[CPG][TILE] = {};
        int nsingle = 0, rows = 0;
        for (int v = 0; v < CPG; ++v) {
            int pre = 0;
            for (int k = v * TILE; k < (v + 1) * TILE; ++k) {
                const Word w = decode(tab[k]);
                CHECK(encode(w) == tab[k]);
                CHECK(w.lt >= 0 && w.lt < TILE && w.cq >= 0 && w.cq < CPG && w.cnt >= 0 && w.cnt <= tm);
                CHECK(w.trips == decode(tab[v * TILE]).trips && w.trips <= tm);
                CHECK(!slot_used[w.cq][w.lt]);
                slot_used[w.cq][w.lt] = true;
                // what the kernel runs for this thread
                const int ell = w.single ? lhi : lhi - 63 + w.lt;
                int m = (w.single ? CPG * g.cg + CPG : CPG * g.cg + w.cq) * tm, cnt = w.cnt;
                const int chunk = m / tm;
                if (w.single) {
                    ++nsingle;
                    CHECK(g.absorb && cnt == 1 && m == lhi);
                    // the slot it stands in for holds no segment
                    CHECK(seg_rows(L, tm, g.tile, g.cg, w.cq, w.lt) == 0);
                } else {
                    CHECK(cnt == seg_rows(L, tm, g.tile, g.cg, w.cq, w.lt));
                }
                int first = m, total = cnt;
                if (cnt > 0 && m == 0) { m = 1; --cnt; pre = 1; }
                CHECK(cnt <= w.trips);
                CHECK(cover(ell, first, total, chunk));
            }
            rows += decode(tab[v * TILE]).trips + pre;
        }
        CHECK(rows == g.rows_issued);
        CHECK(nsingle == (g.absorb ? 1 : 0));
        if (g.absorb) {
            ++nabsorb;
            CHECK(g.cg + 1 < P.nchunkg && lhi == CPG * (g.cg + 1) * tm);
            CHECK(slots.insert({g.tile, g.cg + 1}).second);
        }
    }
    for (int m = 0; m <= L; ++m)
        for (int l = 0; l <= L; ++l) CHECK(seen[(size_t)m * (L + 1) + l] == (m <= l ? 1 : 0));
    // the partial slots written are those of the plain grid
    std::set<std::pair<int, int>> plain;
    for (const Group& g : Q.groups) {
        CHECK(!g.packed && !g.absorb);
        plain.insert({g.tile, g.cg});
    }
    CHECK(plain == slots);
    CHECK(Q.ncls == 0 && Q.table.empty() && Q.rows_issued == Q.rows_plain);
    CHECK(issued == P.rows_issued && P.rows_plain == Q.rows_plain && P.rows_issued <= P.rows_plain);
    CHECK((int)Q.groups.size() == (int)P.groups.size() + nabsorb);
    std::printf("%d %d %d %d %d %lld %lld %d %d\n", L, tm, (int)P.groups.size(), npacked, nabsorb, P.rows_plain,
                P.rows_issued, npacked_m0, npacked_partial);
    return 0;
}

int main(int argc, char** argv) {
    int rc = 0;
    for (int k = 1; k < argc; ++k) rc |= check(std::atoi(argv[k]));
    return rc;
}
