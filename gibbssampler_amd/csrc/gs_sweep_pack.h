// Packed form of the CR sweep's diagonal workgroups: the host-side table
// builder (plain C++, no HIP; tests/sweep_pack_check.cpp builds it alone).
//
// The sweep tiles the (l, m) triangle l >= m: 64-wide l tiles descending from
// l = L (tile t holds l in [L - 64 t - 63, L - 64 t]), rows m in chunks of tm,
// 4 chunks to a chunk group.  With one tile per workgroup (tw = 1) a workgroup
// (tile, chunk group) owns 4 x 64 = 256 column segments (l, chunk): the entries
// (l, m) of the chunk's rows with m <= l, 0 .. tm of them, always starting at
// the chunk's first row.  Off the diagonal all 256 are full and wave w = chunk
// w runs tm rows with every lane busy.  On the diagonal most are short or
// empty, and the plain form still issues every row of every chunk-wave.
//
// The packed form deals the 256 segments over the 256 threads by length,
// longest first: thread k takes the k-th longest, so wave 0 holds the 64
// longest, and each wave's row loop is as long as its own longest segment.
// Every thread still owns exactly one (chunk, l) slot of the workgroup's LDS
// sums (an empty segment gives zeros), so the chunk-group partial is formed
// from the same four terms in the same order as the plain form's.
//
// Absorbed single entry: where a tile's last chunk group holds the one entry
// (l_hi, m = l_hi), the packed workgroup of the chunk group before it gives
// that entry to its first thread with an empty segment and writes the second
// partial slot as well; the one-entry workgroup leaves the grid.
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <vector>

#if defined(__HIPCC__)
#define GS_PACK_HD __host__ __device__
#else
#define GS_PACK_HD
#endif

namespace gs_pack {

constexpr int TILE = 64;        // l per tile = lanes per wave
constexpr int CPG = 4;          // chunks per chunk group = waves per workgroup
constexpr int NTHREAD = TILE * CPG;

// rows per chunk: a function of L only (build_tasks in gs_kernels.hip says why)
inline int rows_per_chunk(int L) { return L > 512 ? 16 : (L > 256 ? 4 : 8); }

// one thread's table word: its LDS slot (lt, cq) = its segment's l-in-tile and
// chunk-in-group, the segment's row count, its wave's row-loop trips (the same
// value in all 64 threads of a wave; row m = 0 is taken before the loop and not
// counted), and whether the thread's work is the absorbed single entry instead
// of its own (empty) segment
struct Word {
    int lt, cq, cnt, trips;
    bool single;
};
GS_PACK_HD inline uint32_t encode(const Word& w) {
    return (uint32_t)w.lt | (uint32_t)w.cq << 6 | (uint32_t)w.cnt << 8 | (uint32_t)w.trips << 13 |
           (uint32_t)(w.single ? 1 : 0) << 18;
}
GS_PACK_HD inline Word decode(uint32_t u) {
    return Word{(int)(u & 63u), (int)(u >> 6 & 3u), (int)(u >> 8 & 31u), (int)(u >> 13 & 31u), (u >> 18 & 1u) != 0};
}

// rows of segment (l-in-tile lt, chunk cq) of workgroup (tile, chunk group cg)
inline int seg_rows(int L, int tm, int tile, int cg, int cq, int lt) {
    const int l = L - TILE * tile - (TILE - 1) + lt;
    const int m0 = (CPG * cg + cq) * tm;
    return l < m0 ? 0 : std::min(tm, l - m0 + 1);       // (l < 0 <= m0: none)
}

// one workgroup of the grid
struct Group {
    int tile = 0, cg = 0;
    bool packed = false;        // runs the packed form (table class cls)
    bool absorb = false;        // ... and the single entry of chunk group cg + 1
    int cls = -1;
    int rows_plain = 0;         // wave-rows the plain form issues for (tile, cg)
    int rows_issued = 0;        // wave-rows this workgroup issues
};

struct Plan {
    int L = 0, tm = 0, ntile = 0, nchunkg = 0;
    std::vector<Group> groups;              // the grid, absorbed groups left out
    std::vector<uint32_t> table;            // [ncls][NTHREAD] thread words
    int ncls = 0;
    long long rows_plain = 0, rows_issued = 0;   // per chain, all workgroups
};

// the words of a packed workgroup and the wave-rows it issues
inline int pack_group(int L, int tm, int tile, int cg, bool absorb, uint32_t (&out)[NTHREAD]) {
    Word w[NTHREAD];
    for (int cq = 0; cq < CPG; ++cq)
        for (int lt = 0; lt < TILE; ++lt)
            w[cq * TILE + lt] = Word{lt, cq, seg_rows(L, tm, tile, cg, cq, lt), 0, false};
    // longest first; ties in slot order (the table is a function of L and tm alone)
    std::stable_sort(w, w + NTHREAD, [](const Word& a, const Word& b) { return a.cnt > b.cnt; });
    if (absorb) {
        int k = 0;
        while (k < NTHREAD && w[k].cnt > 0) ++k;
        if (k == NTHREAD) return -1;                    // no empty segment to carry it
        w[k].cnt = 1;
        w[k].single = true;
    }
    int issued = 0;
    for (int v = 0; v < CPG; ++v) {
        int trips = 0, pre = 0;
        for (int k = v * TILE; k < (v + 1) * TILE; ++k) {
            // row m = 0 (chunk 0 of chunk group 0) is one real slot, taken before the loop
            const int first0 = (!w[k].single && cg == 0 && w[k].cq == 0 && w[k].cnt > 0) ? 1 : 0;
            trips = std::max(trips, w[k].cnt - first0);
            pre = std::max(pre, first0);
        }
        for (int k = v * TILE; k < (v + 1) * TILE; ++k) w[k].trips = trips;
        issued += trips + pre;
    }
    for (int k = 0; k < NTHREAD; ++k) out[k] = encode(w[k]);
    return issued;
}

// the sweep grid of one chain for tw = 1: every (tile, chunk group) with an
// entry, the diagonal ones packed when pack is set
inline Plan build(int L, int tm, bool pack) {
    Plan P;
    P.L = L;
    P.tm = tm;
    P.ntile = (L + TILE) / TILE;
    P.nchunkg = (L / tm + 1 + CPG - 1) / CPG;
    std::map<std::vector<uint32_t>, int> classes;
    for (int t = 0; t < P.ntile; ++t) {
        const int lhi = L - TILE * t;
        for (int c = 0; c * CPG * tm <= lhi; ++c) {
            Group g;
            g.tile = t;
            g.cg = c;
            for (int cq = 0; cq < CPG; ++cq) {
                const int m0 = (CPG * c + cq) * tm;
                g.rows_plain += std::max(0, std::min(m0 + tm, lhi + 1) - m0);
            }
            g.rows_issued = g.rows_plain;
            P.rows_plain += g.rows_plain;
            if (pack) {
                // the next chunk group is the tile's last and holds (l_hi, l_hi) alone
                const bool single_next = lhi == CPG * (c + 1) * tm;
                uint32_t words[NTHREAD];
                int issued = pack_group(L, tm, t, c, single_next, words);
                bool absorb = single_next && issued >= 0;
                if (single_next && !absorb) issued = pack_group(L, tm, t, c, false, words);
                if (absorb || issued < g.rows_plain) {
                    g.packed = true;
                    g.absorb = absorb;
                    g.rows_issued = issued;
                    const std::vector<uint32_t> key(words, words + NTHREAD);
                    auto it = classes.find(key);
                    if (it == classes.end()) {
                        it = classes.emplace(key, P.ncls++).first;
                        P.table.insert(P.table.end(), key.begin(), key.end());
                    }
                    g.cls = it->second;
                }
            }
            P.rows_issued += g.rows_issued;
            P.groups.push_back(g);
            if (g.absorb) {
                P.rows_plain += 1;                      // the absorbed group's one wave-row
                ++c;
            }
        }
    }
    return P;
}

}  // namespace gs_pack
