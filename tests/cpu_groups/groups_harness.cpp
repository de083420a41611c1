// groups_harness.cpp — the host's tables of a grouped world's neighbour search (group_tables, magics_amd/csrc/mgx_search.h) on the
// CPU, as a stand-alone program meant to be built with -fsanitize=address,undefined (tests/test_groups_host.py): members by group,
// ascending within a group; a segment per non-empty group; one (segment, first member) record per GROUP_ROBOTS robots; which
// codes the dispatch helpers answer for.  Prints one line per failed check and returns their number.
#include <cstdio>
#include <vector>

#include "../../magics_amd/csrc/mgx_search.h"

using namespace mgx;

static int failures = 0;
#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            failures++;                                       \
            printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
            printf(__VA_ARGS__);                              \
            printf("\n");                                     \
        }                                                     \
    } while (0)

// everything the kernel relies on, for any query: every robot of the query in exactly one segment, segments of one group, ascending
// within, workgroups that cover every segment in slices of GROUP_ROBOTS, `largest` the largest segment
static void check_tables(const std::vector<uint32_t> &group, const char *what) {
    GroupTables t;
    const int n = (int)group.size();
    const bool ok = group_tables(group.data(), n, t);
    CHECK((int)t.members.size() == n, "%s: %zu members for %d robots", what, t.members.size(), n);
    CHECK(!t.seg.empty() && t.seg.front() == 0 && t.seg.back() == n, "%s: the segments do not span the members", what);
    std::vector<int> seen((size_t)n, 0);
    int largest = 0;
    for (int s = 0; s < t.n_segments(); s++) {
        const int a = t.seg[(size_t)s], b = t.seg[(size_t)s + 1];
        CHECK(b > a, "%s: segment %d is empty", what, s);
        largest = b - a > largest ? b - a : largest;
        for (int q = a; q < b; q++) {
            const int32_t m = t.members[(size_t)q];
            CHECK(m >= 0 && m < n, "%s: member %d out of the query", what, m);
            if (m < 0 || m >= n) continue;
            seen[(size_t)m]++;
            CHECK(group[(size_t)m] == group[(size_t)t.members[(size_t)a]], "%s: segment %d mixes groups", what, s);
            CHECK(q == a || t.members[(size_t)q - 1] < m, "%s: segment %d does not ascend", what, s);
        }
        CHECK(s == 0 || group[(size_t)t.members[(size_t)t.seg[(size_t)s - 1]]] < group[(size_t)t.members[(size_t)a]], "%s: groups out of order at segment %d", what, s);
    }
    for (int q = 0; q < n; q++) CHECK(seen[(size_t)q] == 1, "%s: robot %d is listed %d times", what, q, seen[(size_t)q]);
    CHECK(t.largest == largest, "%s: largest %d, the segments say %d", what, t.largest, largest);
    CHECK(ok == (largest <= ROWS_MAX_N), "%s: a largest group of %d answered %d", what, largest, (int)ok);
    // the workgroups: segment after segment, slices of GROUP_ROBOTS from 0 on
    size_t w = 0;
    for (int s = 0; s < t.n_segments(); s++)
        for (int first = 0; first < t.seg[(size_t)s + 1] - t.seg[(size_t)s]; first += GROUP_ROBOTS, w++) {
            CHECK(2 * w + 1 < t.wg.size(), "%s: too few workgroups", what);
            if (2 * w + 1 < t.wg.size()) CHECK(t.wg[2 * w] == s && t.wg[2 * w + 1] == first, "%s: workgroup %zu is (%d, %d), wanted (%d, %d)", what, w, t.wg[2 * w], t.wg[2 * w + 1], s, first);
        }
    CHECK((size_t)t.n_workgroups() == w, "%s: %d workgroups, wanted %zu", what, t.n_workgroups(), w);
    CHECK(t.off_seg() == t.members.size() && t.off_wg() == t.members.size() + t.seg.size() && t.words() == t.off_wg() + t.wg.size(), "%s: offsets", what);
}

int main() {
    check_tables({}, "an empty query");
    check_tables({0}, "one robot");
    check_tables({5, 3, 9, 0, 7}, "one robot per group");
    check_tables({4, 4, 9, 9, 9, 4}, "groups with gaps (0 .. 3 and 5 .. 8 are empty)");
    {   // ids interleaved: sizes 1, 15, 16, 17 and 33 by turns
        std::vector<uint32_t> g;
        const int sizes[5] = {1, 15, 16, 17, 33};
        for (int i = 0; i < 33; i++)
            for (uint32_t k = 0; k < 5; k++)
                if (i < sizes[k]) g.push_back(k);
        check_tables(g, "interleaved ids");
        GroupTables t;
        group_tables(g.data(), (int)g.size(), t);
        CHECK(t.n_segments() == 5 && t.n_workgroups() == 1 + 1 + 1 + 2 + 3 && t.largest == 33, "interleaved ids: %d segments, %d workgroups", t.n_segments(), t.n_workgroups());
        CHECK(t.members[0] == 0 && t.members[1] == 1 && t.members[2] == 5, "interleaved ids: members start %d %d %d", t.members[0], t.members[1], t.members[2]);
    }
    {   // a group exactly at ROWS_MAX_N beside a small one, and one above it
        std::vector<uint32_t> g((size_t)ROWS_MAX_N, 2u);
        g.push_back(1u);
        check_tables(g, "a group of ROWS_MAX_N");
        GroupTables t;
        CHECK(group_tables(g.data(), (int)g.size(), t) && t.largest == ROWS_MAX_N && t.n_workgroups() == 1 + ROWS_MAX_N / GROUP_ROBOTS, "a group of ROWS_MAX_N is served");
        g.push_back(2u);
        check_tables(g, "a group of ROWS_MAX_N + 1");
        CHECK(!group_tables(g.data(), (int)g.size(), t) && t.largest == ROWS_MAX_N + 1, "a group of ROWS_MAX_N + 1 is refused");
    }
    // the dispatch: a grouped world's query runs MGX_SEARCH_ROWS_GROUPS whatever the method, the size and the radius
    for (uint32_t method = MGX_NEIGHBOURS_AUTO; method <= MGX_NEIGHBOURS_GRID; method++)
        for (int n : {1, 600, 5000}) CHECK(search_kernel_for(n, method, -1.f, 16, true) == MGX_SEARCH_ROWS_GROUPS, "method %u n %d", method, n);
    CHECK(search_kernel_for(0, MGX_NEIGHBOURS_AUTO, 2.f, 16, true) == MGX_SEARCH_NONE, "an empty query launches nothing");
    CHECK(search_kernel_for(600, MGX_NEIGHBOURS_AUTO, 2.f, 16, false) == MGX_SEARCH_ROWS_GRID_16, "an ungrouped world's dispatch is unchanged");
    CHECK(search_in_rows(MGX_SEARCH_ROWS_GROUPS) && !search_keeps_rows(MGX_SEARCH_ROWS_GROUPS), "the grouped kernel writes rows and keeps none");
    CHECK(search_keeps_rows(MGX_SEARCH_ROWS_GRID_16) && search_keeps_rows(MGX_SEARCH_ROWS_GRID_32) && !search_keeps_rows(MGX_SEARCH_ROWS_PAIRS_2) &&
              !search_in_rows(MGX_SEARCH_TWO_PASS_GRID), "the other codes answer as before");
    printf("groups harness: %d failed checks\n", failures);
    return failures;
}
