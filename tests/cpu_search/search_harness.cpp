// search_harness.cpp — the pure host helpers of the neighbour search (magics_amd/csrc/mgx_search.h) on the CPU, as a stand-alone
// program meant to be built with -fsanitize=address,undefined (tests/test_search_host.py): the dispatch against a table written
// out here, rows -> CSR, the mapping of a compacted query back to world ids, the pinned layout.  Prints one line per failed check
// and returns their number.
#include <cstdio>
#include <limits>
#include <numeric>

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

// ---- the dispatch: AUTO, per query size (the sizes of tests/test_gpu_search_matrix.py), per row capacity 16 / 32 / 64, per radius
// 2.0 / 0 / -1 / NaN / inf — what that test's expected_search states for a search that does not outgrow its rows
enum : int32_t { TP = MGX_SEARCH_TWO_PASS_PAIRS, TG = MGX_SEARCH_TWO_PASS_GRID, P4 = MGX_SEARCH_ROWS_PAIRS_4, P2 = MGX_SEARCH_ROWS_PAIRS_2,
                 G16 = MGX_SEARCH_ROWS_GRID_16, G32 = MGX_SEARCH_ROWS_GRID_32 };
struct Entry { int n; int32_t want[3][5]; };
static const Entry TABLE[] = {
    {1, {{G16, P4, P4, P4, P4}, {G32, P4, P4, P4, P4}, {P4, P4, P4, P4, P4}}},
    {2, {{G16, P4, P4, P4, P4}, {G32, P4, P4, P4, P4}, {P4, P4, P4, P4, P4}}},
    {3, {{G16, P4, P4, P4, P4}, {G32, P4, P4, P4, P4}, {P4, P4, P4, P4, P4}}},
    {5, {{G16, P4, P4, P4, P4}, {G32, P4, P4, P4, P4}, {P4, P4, P4, P4, P4}}},
    {6, {{G16, P4, P4, P4, P4}, {G32, P4, P4, P4, P4}, {P4, P4, P4, P4, P4}}},
    {7, {{G16, P4, P4, P4, P4}, {G32, P4, P4, P4, P4}, {P4, P4, P4, P4, P4}}},
    {63, {{G16, P4, P4, P4, P4}, {G32, P4, P4, P4, P4}, {P4, P4, P4, P4, P4}}},
    {64, {{G16, P4, P4, P4, P4}, {G32, P4, P4, P4, P4}, {P4, P4, P4, P4, P4}}},
    {65, {{G16, P4, P4, P4, P4}, {G32, P4, P4, P4, P4}, {P4, P4, P4, P4, P4}}},
    {127, {{G16, P4, P4, P4, P4}, {G32, P4, P4, P4, P4}, {P4, P4, P4, P4, P4}}},
    {128, {{G16, P4, P4, P4, P4}, {G32, P4, P4, P4, P4}, {P4, P4, P4, P4, P4}}},
    {129, {{G16, P4, P4, P4, P4}, {G32, P4, P4, P4, P4}, {P4, P4, P4, P4, P4}}},
    {511, {{G16, P4, P4, P4, P4}, {G32, P4, P4, P4, P4}, {P4, P4, P4, P4, P4}}},
    {512, {{G16, P4, P4, P4, P4}, {G32, P4, P4, P4, P4}, {P4, P4, P4, P4, P4}}},
    {513, {{G16, P2, P2, P2, P2}, {G32, P2, P2, P2, P2}, {P2, P2, P2, P2, P2}}},
    {1000, {{G16, P2, P2, P2, P2}, {G32, P2, P2, P2, P2}, {P2, P2, P2, P2, P2}}},
    {1023, {{G16, P2, P2, P2, P2}, {G32, P2, P2, P2, P2}, {P2, P2, P2, P2, P2}}},
    {1024, {{G16, P2, P2, P2, P2}, {G32, P2, P2, P2, P2}, {P2, P2, P2, P2, P2}}},
    {1025, {{P4, P4, P4, P4, P4}, {P4, P4, P4, P4, P4}, {P4, P4, P4, P4, P4}}},
    {4096, {{P4, P4, P4, P4, P4}, {P4, P4, P4, P4, P4}, {P4, P4, P4, P4, P4}}},
    {4097, {{TG, TP, TP, TP, TP}, {TG, TP, TP, TP, TP}, {TG, TP, TP, TP, TP}}},
};

static void check_dispatch() {
    const int caps[3] = {16, 32, 64};
    const float radii[5] = {2.0f, 0.0f, -1.0f, std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity()};
    for (const Entry &e : TABLE)
        for (int c = 0; c < 3; c++)
            for (int r = 0; r < 5; r++) {
                const int32_t got = search_kernel_for(e.n, MGX_NEIGHBOURS_AUTO, radii[r], caps[c]);
                CHECK(got == e.want[c][r], "n %d cap %d radius %g: kernel %d, the table says %d", e.n, caps[c], (double)radii[r], got, e.want[c][r]);
                CHECK(search_in_rows(got) == (e.n <= 4096) && search_keeps_rows(got) == (got == G16 || got == G32), "n %d: kind of kernel %d", e.n, got);
                // a method asked for by name is the two-pass form of it, whatever the size; a grid needs a usable radius
                CHECK(search_kernel_for(e.n, MGX_NEIGHBOURS_PAIRS, radii[r], caps[c]) == TP, "n %d PAIRS", e.n);
                CHECK(search_kernel_for(e.n, MGX_NEIGHBOURS_GRID, radii[r], caps[c]) == (r == 0 ? TG : TP), "n %d GRID radius %g", e.n, (double)radii[r]);
            }
    CHECK(search_kernel_for(0, MGX_NEIGHBOURS_AUTO, 2.0f, 16) == MGX_SEARCH_NONE && !search_in_rows(MGX_SEARCH_NONE), "an empty query");
}

// ---- rows of a fixed capacity -> CSR ----------------------------------------------------------------------------------------------
// rows[i * cap + k] = 1000 i + k for k < min(cnt[i], cap); beyond that a poison the CSR must never show
static void check_rows_case(const std::vector<int32_t> &cnt, int cap, const std::vector<uint8_t> *mask) {
    const int n = (int)cnt.size();
    const int32_t POISON = -77;
    std::vector<int32_t> rows((size_t)n * (size_t)cap, POISON);   // exactly n x cap: a read past the end is the sanitizer's to report
    for (int i = 0; i < n; i++)
        for (int k = 0; k < cnt[(size_t)i]; k++) rows[(size_t)i * (size_t)cap + (size_t)k] = 1000 * i + k;
    std::vector<int32_t> ptr{5, 5, 5}, idx(3, POISON);   // (what the caller's vectors held before is gone)
    rows_to_csr(cnt.data(), rows.data(), n, cap, mask ? mask->data() : nullptr, ptr, idx);
    CHECK((int)ptr.size() == n + 1 && ptr[0] == 0, "ptr has %zu entries for %d rows", ptr.size(), n);
    int32_t total = 0;
    for (int i = 0; i < n; i++) {
        CHECK(ptr[(size_t)i + 1] - ptr[(size_t)i] == cnt[(size_t)i], "row %d of %d: length", i, n);
        total += cnt[(size_t)i];
        if (mask && !(*mask)[(size_t)i]) continue;   // (left out: not to be read)
        for (int k = 0; k < cnt[(size_t)i]; k++)
            CHECK(idx[(size_t)ptr[(size_t)i] + (size_t)k] == 1000 * i + k, "row %d entry %d (n %d cap %d mask %d)", i, k, n, cap, mask != nullptr);
    }
    CHECK((int32_t)idx.size() == total && ptr[(size_t)n] == total, "total %d, idx holds %zu", total, idx.size());
}
static void check_rows_to_csr() {
    for (int cap : {1, 16, 32}) {
        const std::vector<std::vector<int32_t>> cases = {
            {0}, {1}, {cap},                                   // n = 1: empty, one entry, full
            {0, 0, 0}, {1, 1, 1, 1}, {cap, cap, cap},          // all empty, all one, all full
            {0, cap, 1, 0, cap, cap > 1 ? cap - 1 : 1, 0},     // mixed, empty rows first, last and in between
            {cap, 0}, {0, cap},
        };
        for (const auto &cnt : cases) {
            check_rows_case(cnt, cap, nullptr);
            const int n = (int)cnt.size();
            for (unsigned pattern : {0u, ~0u, 0x55555555u, 0xaaaaaaaau, 1u, 1u << (n - 1)}) {
                std::vector<uint8_t> mask((size_t)n);
                for (int i = 0; i < n; i++) mask[(size_t)i] = (pattern >> i) & 1u;
                check_rows_case(cnt, cap, &mask);
            }
        }
    }
    // the flags come out of the counts before the rows are laid out
    std::vector<int32_t> cnt = {3 | NEIGHBOURS_CHANGED, 0, NEIGHBOURS_CHANGED, 16, 32 | NEIGHBOURS_CHANGED};
    std::vector<uint8_t> chg(cnt.size(), 9);
    strip_changed(cnt.data(), (int)cnt.size(), chg.data());
    CHECK((cnt == std::vector<int32_t>{3, 0, 0, 16, 32}) && (chg == std::vector<uint8_t>{1, 0, 1, 0, 1}), "strip_changed");
}

// ---- a compacted query back to world ids ------------------------------------------------------------------------------------------
static void check_compact_case(int n_all, const std::vector<int> &removed) {
    std::vector<uint8_t> gone((size_t)n_all, 0);
    for (int r : removed) gone[(size_t)r] = 1;
    std::vector<int> alive;
    for (int r = 0; r < n_all; r++)
        if (!gone[(size_t)r]) alive.push_back(r);
    const int n = (int)alive.size();
    // query row a: every other query robot b with (a + b) % 3 == 0, ascending
    std::vector<int32_t> ptr{0}, idx;
    for (int a = 0; a < n; a++) {
        for (int b = 0; b < n; b++)
            if (b != a && (a + b) % 3 == 0) idx.push_back(b);
        ptr.push_back((int32_t)idx.size());
    }
    const std::vector<int32_t> qptr = ptr, qidx = idx;
    compact_to_world(alive, n_all, ptr, idx);
    CHECK((int)ptr.size() == n_all + 1 && ptr[0] == 0 && ptr[(size_t)n_all] == (int32_t)qidx.size() && idx.size() == qidx.size(), "compact: sizes (%d robots, %zu removed)", n_all, removed.size());
    int a = 0;
    for (int r = 0; r < n_all; r++) {
        const int32_t len = ptr[(size_t)r + 1] - ptr[(size_t)r];
        if (gone[(size_t)r]) { CHECK(len == 0, "compact: removed robot %d has a row of %d", r, len); continue; }
        CHECK(len == qptr[(size_t)a + 1] - qptr[(size_t)a] && ptr[(size_t)r] == qptr[(size_t)a], "compact: robot %d, query row %d", r, a);
        for (int32_t k = 0; k < len; k++) {
            const int32_t j = idx[(size_t)ptr[(size_t)r] + (size_t)k];
            CHECK(j == alive[(size_t)qidx[(size_t)qptr[(size_t)a] + (size_t)k]] && !gone[(size_t)j], "compact: robot %d entry %d is %d", r, k, j);
        }
        a++;
    }
}
static void check_compact() {
    check_compact_case(9, {0});            // first
    check_compact_case(9, {8});            // last
    check_compact_case(9, {3, 4});         // adjacent
    check_compact_case(9, {0, 1, 7, 8});   // adjacent at both ends
    check_compact_case(9, {0, 4, 5, 8});
    check_compact_case(2, {0});
    check_compact_case(2, {1});
    check_compact_case(1, {0});            // nobody left
    check_compact_case(65, {0, 31, 32, 33, 64});
}

// ---- the pinned layout -------------------------------------------------------------------------------------------------------------
static void check_layout() {
    for (int n : {1, 2, 3, 5, 63, 64, 65, 1000, 1024, 4096})
        for (int cap : {16, 32, 64, 4096}) {
            const RowsLayout L = rows_layout(n, cap);
            CHECK(L.off_cnt % 4 == 0 && L.off_rows % 4 == 0 && L.bytes % 4 == 0, "layout %d x %d: alignment", n, cap);
            CHECK(L.off_cnt >= sizeof(float) * 3 * (size_t)n, "layout %d x %d: the counts overlap the positions", n, cap);
            CHECK(L.off_rows >= L.off_cnt + sizeof(int32_t) * (size_t)n, "layout %d x %d: the rows overlap the counts", n, cap);
            CHECK(L.bytes >= L.off_rows + sizeof(int32_t) * (size_t)n * (size_t)cap, "layout %d x %d: the rows do not fit", n, cap);
        }
    CHECK(pairs_rows_lds(ROWS_MAX_N) <= 48u * 1024u && pairs_rows_lds(ROWS_MAX_N + 4) > 48u * 1024u, "the largest one-pass query is what 48 KB of LDS hold");
}

int main() {
    check_dispatch();
    check_rows_to_csr();
    check_compact();
    check_layout();
    printf("search harness: %d failed checks\n", failures);
    return failures ? 1 : 0;
}
