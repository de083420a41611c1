// mgx_search.h — what the kernels of the comms-range neighbour search (mgx_topology.hip) and the host that drives them
// (mgx_world_topology.inc) have to agree on: the dispatch constants, which kernel a search runs, the host's pure helpers and the
// launchers' prototypes.  Everything above the prototypes is free of HIP and compiles with a plain C++17 compiler
// (tests/cpu_search/search_harness.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/mgx.h"

namespace mgx {

// ---- the dispatch ---------------------------------------------------------------------------------------------------------------
constexpr int ROWS_MAX_N = 4096;          // largest query of the one-pass search (AUTO): rows of a fixed capacity, written in place
constexpr int GRID_M = 1024;              // buckets of the hash grid in LDS (k_grid_rows) — and its largest query: robot numbers are 16-bit words there
constexpr int GRID_ROWS_MAX_CAP = 32;     // largest row capacity of k_grid_rows (the rows are sorted in registers)
constexpr int TWO_PASS_GRID_MIN_N = 512;  // AUTO, two passes: the hash grid in device memory from here on, all pairs below
constexpr int PAIRS_2_MIN_N = 513, PAIRS_2_MAX_N = 1024;  // k_pairs_rows<2, 128>: the worlds that fill the device with their resident launch
constexpr int GROUP_ROBOTS = 16;           // k_group_rows: robots of ONE group a workgroup serves (four lanes each), 256 candidates per pass
constexpr int NEIGHBOURS_PREV_STRIDE = 33;       // words per robot of the kept rows: count, then up to 32 entries
constexpr int32_t NEIGHBOURS_CHANGED = 1 << 30;  // in a robot's count: its row is not the one of the search before
// the all-pairs rows kernel holds ALL positions in LDS (structure of arrays, padded to four robots)
constexpr size_t pairs_rows_lds(int n) { return sizeof(float) * 3 * (size_t)((n + 3) & ~3); }
static_assert(pairs_rows_lds(ROWS_MAX_N) <= 48 * 1024, "the one-pass search's largest query has to fit 48 KB of LDS");
static_assert(NEIGHBOURS_PREV_STRIDE == 1 + GRID_ROWS_MAX_CAP && GRID_M <= ROWS_MAX_N && PAIRS_2_MAX_N <= ROWS_MAX_N, "dispatch constants");

inline bool usable_radius(float radius) { return std::isfinite(radius) && radius > 0.f; }  // (else every pair has to see the predicate)

// what the one-pass kernels compare squared distances with (in_comms_range_sq, mgx_topology.hip): the largest f32 s with
// RN_f32(sqrt(s)) <= radius; NaN radius -> NaN (everybody in range), radius < 0 -> negative (nobody but NaN distances)
inline float squared_threshold(float radius) {
    if (radius != radius) return radius;
    if (radius < 0.f) return -1.f;
    if (std::isinf(radius)) return radius;
    auto root = [](float s) { return (float)std::sqrt((double)s); };
    float s = (float)((double)radius * (double)radius);
    if (std::isinf(s)) s = std::numeric_limits<float>::max();
    while (root(s) > radius) s = std::nextafter(s, -1.f);
    for (;;) {
        const float up = std::nextafter(s, std::numeric_limits<float>::infinity());
        if (std::isinf(up) || root(up) > radius) break;
        s = up;
    }
    return s;
}

// the kernel (MGX_SEARCH_*) that answers a query of n robots — the one launched LAST where a search takes several launches.
// grouped: the world has robots of a non-zero group (include/mgx.h, ROBOT GROUPS) — one kernel, whatever the method and the size
inline int32_t search_kernel_for(int n, uint32_t method, float radius, int32_t cap, bool grouped = false) {
    if (n <= 0) return MGX_SEARCH_NONE;  // (an empty query launches nothing)
    if (grouped) return MGX_SEARCH_ROWS_GROUPS;
    if (method == MGX_NEIGHBOURS_AUTO && n <= ROWS_MAX_N) {  // small worlds: ONE small kernel, no scans
        if (n <= GRID_M && cap <= GRID_ROWS_MAX_CAP && usable_radius(radius)) return cap <= 16 ? MGX_SEARCH_ROWS_GRID_16 : MGX_SEARCH_ROWS_GRID_32;
        return n >= PAIRS_2_MIN_N && n <= PAIRS_2_MAX_N ? MGX_SEARCH_ROWS_PAIRS_2 : MGX_SEARCH_ROWS_PAIRS_4;
    }
    const bool grid = method == MGX_NEIGHBOURS_GRID || (method == MGX_NEIGHBOURS_AUTO && n >= TWO_PASS_GRID_MIN_N);
    return grid && usable_radius(radius) ? MGX_SEARCH_TWO_PASS_GRID : MGX_SEARCH_TWO_PASS_PAIRS;
}
inline bool search_in_rows(int32_t kernel) { return kernel >= MGX_SEARCH_ROWS_PAIRS_4; }   // one pass, rows of a fixed capacity
inline bool search_keeps_rows(int32_t kernel) { return kernel == MGX_SEARCH_ROWS_GRID_16 || kernel == MGX_SEARCH_ROWS_GRID_32; }  // ... and it can compare them with the kept ones
static_assert(MGX_SEARCH_ROWS_PAIRS_4 == 2 && MGX_SEARCH_ROWS_PAIRS_2 == 3 && MGX_SEARCH_ROWS_GRID_16 == 4 && MGX_SEARCH_ROWS_GRID_32 == 5 &&
                  MGX_SEARCH_ROWS_GROUPS == 6, "order of the codes");

// ---- the host's side of a one-pass search ---------------------------------------------------------------------------------------
// the mapped pinned block the kernel reads and writes in place: [3 n floats: positions up] [n ints: counts down] [n x cap ints: rows down]
struct RowsLayout { size_t off_cnt, off_rows, bytes; };
inline RowsLayout rows_layout(int n, int cap) {
    const size_t off_cnt = sizeof(float) * 3 * (size_t)n, off_rows = off_cnt + sizeof(int32_t) * (size_t)n;
    return {off_cnt, off_rows, off_rows + sizeof(int32_t) * (size_t)n * (size_t)cap};
}
// the changed-row flags out of the counts, one byte per robot
inline void strip_changed(int32_t *cnt, int n, uint8_t *chg) {
    for (int i = 0; i < n; i++) { chg[i] = (cnt[i] & NEIGHBOURS_CHANGED) ? 1 : 0; cnt[i] &= ~NEIGHBOURS_CHANGED; }
}
// rows of a fixed capacity -> CSR.  only_these (may be null): one byte per robot — the rows of the others are left out of idx
// (their places are there, their entries are not to be read)
inline void rows_to_csr(const int32_t *cnt, const int32_t *rows, int n, int cap, const uint8_t *only_these, std::vector<int32_t> &ptr,
                        std::vector<int32_t> &idx) {
    ptr.assign((size_t)n + 1, 0);
    for (int i = 0; i < n; i++) ptr[(size_t)i + 1] = ptr[(size_t)i] + cnt[i];
    idx.resize((size_t)ptr[(size_t)n]);
    for (int i = 0; i < n; i++)
        if (cnt[i] && (!only_these || only_these[i])) memcpy(idx.data() + ptr[(size_t)i], rows + (size_t)i * (size_t)cap, sizeof(int32_t) * (size_t)cnt[i]);
}
// the result of a query over the alive robots only (alive: their world ids, ascending) back to world ids, empty rows for the others
inline void compact_to_world(const std::vector<int> &alive, int n_all, std::vector<int32_t> &ptr, std::vector<int32_t> &idx) {
    for (int32_t &j : idx) j = alive[(size_t)j];
    ptr.resize((size_t)n_all + 1);
    size_t below = alive.size();  // alive robots with an id below r: world row r starts where query row `below` did
    for (int r = n_all; r >= 0; r--) {  // (in place, from the back: below <= r)
        while (below > 0 && alive[below - 1] >= r) below--;
        ptr[(size_t)r] = ptr[below];
    }
}

// ---- a grouped world's search: the query listed by group ---------------------------------------------------------------------
// What k_group_rows reads beside the positions, built by the host when robots join or leave the query:
//   members  the query's robots (indices INTO THE QUERY), group after group, ascending within a group — so rows come out ascending
//   seg      [n_segments + 1] where each non-empty group's members start (a group nobody of the query is in has no segment)
//   wg       [n_workgroups][2] (segment, first member of the slice within the segment): GROUP_ROBOTS robots of one group each
//   largest  the largest segment: sizes the kernel's LDS
//   thr      [n_segments] the squared threshold (squared_threshold) of each SEGMENT's group: the comms radius is per group, and a
//            workgroup reads the one of its segment — listed by segment like seg, so a group without a segment shifts nobody's
//            (group_thresholds, below: filled when a radius changes or the segments do; seg_group and seg_radius stay on the host)
struct GroupTables {
    std::vector<int32_t> members, seg, wg;
    int largest = 0;
    std::vector<uint32_t> seg_group;  // [n_segments] the group every segment lists
    std::vector<float> seg_radius;    // [n_segments] the radius thr was made from
    std::vector<float> thr;
    int n_segments() const { return seg.empty() ? 0 : (int)seg.size() - 1; }
    int n_workgroups() const { return (int)(wg.size() / 2); }
    // the three tables behind one another, as the device holds them: [members n] [seg n_segments + 1] [wg 2 n_workgroups]
    size_t off_seg() const { return members.size(); }
    size_t off_wg() const { return members.size() + seg.size(); }
    size_t words() const { return members.size() + seg.size() + wg.size(); }
    // ... and the thresholds behind them (their bits, one word each): [thr n_segments]
    size_t off_thr() const { return words(); }
    size_t words_with_thr() const { return words() + thr.size(); }
};
// group_of_query [n]: the group of every robot of the query, in query order.  false: a group has more than ROWS_MAX_N robots (no
// workgroup holds its positions) — t.largest says how many
inline bool group_tables(const uint32_t *group_of_query, int n, GroupTables &t) {
    t.members.resize((size_t)std::max(n, 0));
    for (int q = 0; q < n; q++) t.members[(size_t)q] = q;
    std::stable_sort(t.members.begin(), t.members.end(), [&](int32_t a, int32_t b) { return group_of_query[a] < group_of_query[b]; });
    t.seg.assign(1, 0);
    t.wg.clear();
    t.largest = 0;
    t.seg_group.clear();
    t.seg_radius.clear();  // (the segments are new ones: group_thresholds fills thr again)
    t.thr.clear();
    for (int q = 0; q < n;) {
        int e = q + 1;
        while (e < n && group_of_query[t.members[(size_t)e]] == group_of_query[t.members[(size_t)q]]) e++;
        const int32_t segment = (int32_t)t.seg.size() - 1;
        for (int first = 0; first < e - q; first += GROUP_ROBOTS) { t.wg.push_back(segment); t.wg.push_back(first); }
        t.seg.push_back(e);
        t.seg_group.push_back(group_of_query[t.members[(size_t)q]]);
        t.largest = std::max(t.largest, e - q);
        q = e;
    }
    return t.largest <= ROWS_MAX_N;
}
// The thresholds of the tables' segments: radii [n_radii] by GROUP id (a group beyond them, or radii null: `radius`).  false: they
// are the ones the tables hold already (the same radii bit for bit, a NaN included) — nothing to upload
inline bool group_thresholds(GroupTables &t, const float *radii, size_t n_radii, float radius) {
    const size_t ns = t.seg_group.size();
    std::vector<float> now(ns);
    for (size_t s = 0; s < ns; s++) now[s] = radii && t.seg_group[s] < n_radii ? radii[t.seg_group[s]] : radius;
    if (t.thr.size() == ns && t.seg_radius.size() == ns && (ns == 0 || memcmp(now.data(), t.seg_radius.data(), sizeof(float) * ns) == 0)) return false;
    t.thr.resize(ns);
    for (size_t s = 0; s < ns; s++) t.thr[s] = squared_threshold(now[s]);
    t.seg_radius.swap(now);
    return true;
}

// ---- the launchers (mgx_topology.hip) ---------------------------------------------------------------------------------------------
// the two-pass search's scratch, all on the device: cnt[n], bucket_cnt[M], bucket_ptr[M + 1], cursor[M], members[n], special[n],
// n_special[1], ptr[n + 1]
struct SearchScratch { int32_t *cnt, *bucket_cnt, *bucket_ptr, *cursor, *members, *special, *n_special, *ptr; };
#ifdef __HIPCC__
hipError_t neighbours_count(const float *pos, int n, float radius, bool grid, uint32_t M, const SearchScratch &scratch, hipStream_t s);
hipError_t neighbours_fill(const float *pos, int n, float radius, bool grid, uint32_t M, const SearchScratch &scratch, int32_t *idx, int32_t cap,
                           hipStream_t s);
hipError_t neighbours_rows(const float *pos, int n, float radius, int32_t cap, int32_t *cnt, int32_t *rows, hipStream_t s,
                           int32_t *prev = nullptr, int prev_valid = 0, bool *flagged = nullptr, int32_t *ran = nullptr);
// a grouped world's search: tables = GroupTables on the device (members, seg, wg, thr behind one another), largest <= ROWS_MAX_N
hipError_t neighbours_rows_groups(const float *pos, int n, const int32_t *members, const int32_t *seg, const int32_t *wg, int n_workgroups,
                                  int largest, const float *thr, int32_t cap, int32_t *cnt, int32_t *rows, hipStream_t s, int32_t *ran = nullptr);
#endif

}  // namespace mgx
