// plan_harness.cpp — the plan arithmetic of one GBP iteration schedule per robot group (plan_group_launches, group_steps_equal,
// group_steps_check: magics_amd/csrc/mgx_resident.h) on the CPU, as a stand-alone program meant to be built with
// -fsanitize=address,undefined (tests/test_group_schedules_host.py), in the manner of tests/cpu_resident/resident_harness.cpp: equal
// plans, ragged segment counts, an empty group, external-only segments, hints that are true per group, 1 and MGX_GROUPS_MAX groups —
// each against values written out here by hand.  The arrays handed in are exactly as long as the call says, on the heap: a byte read
// beside them is the sanitizer's to report.  Prints one line per failed check and returns their number.
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <memory>

#include "../../magics_amd/csrc/mgx_resident.h"

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

constexpr uint8_t I = 1, E = 2, IE = 3;
constexpr uint32_t EXT = 3u, INT = 12u;                       // both external phases / both internal phases of a segment
constexpr uint32_t DEAD = 1u, LATER_E = 2u, LATER_I = 4u;     // HINT_IR_DEAD, HINT_LATER_EXT_VARIABLE, HINT_LATER_INT_VARIABLE

// per-group schedules packed as the ABI takes them, in arrays of exactly the right length
struct Packed {
    uint32_t n_groups;
    std::unique_ptr<uint8_t[]> steps;
    std::unique_ptr<uint32_t[]> first;
    Packed(std::initializer_list<std::vector<uint8_t>> groups) : n_groups((uint32_t)groups.size()), first(new uint32_t[groups.size() + 1]) {
        size_t total = 0;
        for (const auto &g : groups) total += g.size();
        steps.reset(total ? new uint8_t[total] : nullptr);
        uint32_t at = 0, gi = 0;
        for (const auto &g : groups) {
            first[gi++] = at;
            if (!g.empty()) memcpy(steps.get() + at, g.data(), g.size());
            at += (uint32_t)g.size();
        }
        first[gi] = at;
    }
    GroupPlan plan() const { return plan_group_launches(n_groups, steps.get(), first.get()); }
};
static bool same(const GroupSeg &s, uint32_t ext, uint32_t in, int n_int, uint32_t hints) {
    return s.ext_mask == ext && s.int_mask == in && s.n_int == n_int && s.hints == hints;
}
static void show(const char *what, const GroupPlan &p) {
    for (size_t k = 0; k < p.n_launches; k++)
        for (uint32_t g = 0; g < p.n_groups; g++) {
            const GroupSeg &s = p.launch(k)[g];
            printf("  %s launch %zu group %u: ext %u int %u n_int %d hints %u\n", what, k, g, s.ext_mask, s.int_mask, s.n_int, s.hints);
        }
}

// ---- the single schedule's flattening, as ever (plan_launches moved into the header with this work): interleave-evenly 3 / 3
static void check_plan_launches() {
    const uint8_t steps[3] = {IE, IE, IE};  // I E I E I E -> [I] [E I] [E I] [E]
    const std::vector<Launch> p = plan_launches(steps, 3);
    CHECK(p.size() == 4, "%zu segments", p.size());
    if (p.size() != 4) return;
    CHECK(p[0].ext == 0 && p[0].n_int == 1 && p[0].hints == (LATER_E | LATER_I), "segment 0: %u %d %u", p[0].ext, p[0].n_int, p[0].hints);
    CHECK(p[1].ext == EXT && p[1].n_int == 1 && p[1].hints == (DEAD | LATER_E | LATER_I), "segment 1: %u %d %u", p[1].ext, p[1].n_int, p[1].hints);
    CHECK(p[2].ext == EXT && p[2].n_int == 1 && p[2].hints == (DEAD | LATER_E), "segment 2: %u %d %u", p[2].ext, p[2].n_int, p[2].hints);
    CHECK(p[3].ext == EXT && p[3].n_int == 0 && p[3].hints == 0u, "segment 3: %u %d %u", p[3].ext, p[3].n_int, p[3].hints);
    CHECK(plan_launches(nullptr, 0).empty(), "no steps, no launches");
    const uint8_t idle_steps[2] = {0, 0};
    CHECK(plan_launches(idle_steps, 2).empty(), "steps without a phase, no launches");
}

// ---- equal plans: every launch carries the same record for every group, and the groups ARE equal
static void check_equal() {
    const Packed a{{IE, I, IE}, {IE, I, IE}, {IE, I, IE}};  // I E I I E -> [I] [E I I] [E]
    const GroupPlan p = a.plan();
    CHECK(p.n_launches == 3 && p.n_groups == 3 && p.recs.size() == 9, "%zu launches", p.n_launches);
    if (p.n_launches != 3) return;
    for (uint32_t g = 0; g < 3; g++) {
        const bool ok = same(p.launch(0)[g], 0, INT, 1, LATER_E | LATER_I) && same(p.launch(1)[g], EXT, INT, 2, DEAD | LATER_E) && same(p.launch(2)[g], EXT, 0, 0, 0);
        CHECK(ok && p.n_segments[g] == 3, "group %u", g);
        if (!ok) show("equal", p);
    }
    CHECK(p.writes_snap[0] && p.writes_snap[1] && !p.writes_snap[2], "snapshots: %d %d %d", p.writes_snap[0], p.writes_snap[1], p.writes_snap[2]);
    CHECK(!p.any_ext[0] && p.any_ext[1] && p.any_ext[2], "external: %d %d %d", p.any_ext[0], p.any_ext[1], p.any_ext[2]);
    const uint8_t live[3] = {1, 1, 1};
    uint32_t first = 99;
    CHECK(group_steps_equal(3, a.steps.get(), a.first.get(), live, &first) && first == 0, "equal groups are equal (first %u)", first);
}

// ---- ragged segment counts, an empty group and external-only segments in one call.  Group 0: internal 1 / external 4 the way
// interleave-evenly lays it out (E E IE E: the reference's experiment has such schedules); group 1: two internal iterations;
// group 2: nothing; group 3: late-as-possible 2 / 2 (I I E ... as steps IE IE)
static void check_ragged() {
    const Packed a{{E, E, IE, E}, {I, I}, {}, {IE, IE}};
    const GroupPlan p = a.plan();
    // group 0: E E I E E -> [E] [E I] [E] [E];  group 1: [I I];  group 3: I E I E -> [I] [E I] [E]
    CHECK(p.n_launches == 4 && p.n_groups == 4, "%zu launches", p.n_launches);
    if (p.n_launches != 4) return;
    CHECK(p.n_segments[0] == 4 && p.n_segments[1] == 1 && p.n_segments[2] == 0 && p.n_segments[3] == 3, "segment counts %u %u %u %u", p.n_segments[0],
          p.n_segments[1], p.n_segments[2], p.n_segments[3]);
    bool ok = same(p.launch(0)[0], EXT, 0, 0, DEAD | LATER_E | LATER_I) && same(p.launch(1)[0], EXT, INT, 1, DEAD | LATER_E) &&
              same(p.launch(2)[0], EXT, 0, 0, DEAD | LATER_E) && same(p.launch(3)[0], EXT, 0, 0, 0);
    CHECK(ok, "group 0: external-only segments, hints from its OWN later segments");
    ok = ok && same(p.launch(0)[1], 0, INT, 2, 0);
    CHECK(same(p.launch(0)[1], 0, INT, 2, 0), "group 1: one segment, no promise about a later one (the other groups' do not count)");
    for (size_t k = 1; k < 4; k++) {
        CHECK(sits_out(p.launch(k)[1]) && same(p.launch(k)[1], 0, 0, 0, 0), "group 1 sits launch %zu out", k);
        ok = ok && sits_out(p.launch(k)[1]);
    }
    for (size_t k = 0; k < 4; k++) {
        CHECK(sits_out(p.launch(k)[2]) && same(p.launch(k)[2], 0, 0, 0, 0), "the empty group sits launch %zu out", k);
        ok = ok && sits_out(p.launch(k)[2]);
    }
    const bool g3 = same(p.launch(0)[3], 0, INT, 1, LATER_E | LATER_I) && same(p.launch(1)[3], EXT, INT, 1, DEAD | LATER_E) && same(p.launch(2)[3], EXT, 0, 0, 0) &&
                    sits_out(p.launch(3)[3]);
    CHECK(g3, "group 3");
    if (!ok || !g3) show("ragged", p);
    // launch 0 writes snapshots (groups 1 and 3 run internal sweeps) while group 0 runs an external iteration only; launch 2 and 3
    // write none
    CHECK(p.writes_snap[0] && p.writes_snap[1] && !p.writes_snap[2] && !p.writes_snap[3], "snapshots %d %d %d %d", p.writes_snap[0], p.writes_snap[1],
          p.writes_snap[2], p.writes_snap[3]);
    CHECK(p.any_ext[0] && p.any_ext[1] && p.any_ext[2] && p.any_ext[3], "external phases");
    CHECK(!sits_out(p.launch(0)[0]) && !sits_out(p.launch(0)[1]), "a segment with a phase does not sit out");
    // which groups are live decides whether the call is the plain one
    uint32_t first = 99;
    const uint8_t all[4] = {1, 1, 1, 1}, only1[4] = {0, 1, 0, 0}, none[4] = {0, 0, 0, 0}, empty_and_1[4] = {0, 1, 1, 0};
    CHECK(!group_steps_equal(4, a.steps.get(), a.first.get(), all, &first), "different schedules are not equal");
    CHECK(group_steps_equal(4, a.steps.get(), a.first.get(), only1, &first) && first == 1, "one live group: its steps (first %u)", first);
    CHECK(group_steps_equal(4, a.steps.get(), a.first.get(), none, &first) && first == 4, "no live group: nothing to run (first %u)", first);
    CHECK(!group_steps_equal(4, a.steps.get(), a.first.get(), empty_and_1, &first), "an empty range against a schedule");
    // the same lengths, one byte apart
    const Packed b{{IE, I}, {IE, E}};
    const uint8_t two[2] = {1, 1};
    CHECK(!group_steps_equal(2, b.steps.get(), b.first.get(), two, &first), "equal lengths, different bytes");
}

// ---- 1 group and MGX_GROUPS_MAX (4096) groups
static void check_sizes() {
    const Packed one{{IE, IE}};
    const GroupPlan p1 = one.plan();
    CHECK(p1.n_launches == 3 && p1.recs.size() == 3 && same(p1.launch(1)[0], EXT, INT, 1, DEAD | LATER_E), "one group");
    const uint8_t l1[1] = {1};
    uint32_t first = 99;
    CHECK(group_steps_equal(1, one.steps.get(), one.first.get(), l1, &first) && first == 0, "one group is equal to itself");
    constexpr uint32_t N = 4096;
    std::unique_ptr<uint32_t[]> sf(new uint32_t[N + 1]);
    size_t total = 0;
    for (uint32_t g = 0; g < N; g++) { sf[g] = (uint32_t)total; total += g % 5; }  // 0 .. 4 steps: every fifth group is empty
    sf[N] = (uint32_t)total;
    std::unique_ptr<uint8_t[]> st(new uint8_t[total]);
    for (uint32_t g = 0; g < N; g++)
        for (uint32_t i = 0; i < g % 5; i++) st[sf[g] + i] = (uint8_t)(1 + (g + i) % 3);  // I, E or IE
    const GroupPlan p = plan_group_launches(N, st.get(), sf.get());
    CHECK(p.n_groups == N && p.recs.size() == p.n_launches * N && p.n_launches > 0 && p.n_launches <= 8, "%zu launches", p.n_launches);
    size_t bad = 0, segs = 0;
    for (uint32_t g = 0; g < N; g++) {
        const std::vector<Launch> own = plan_launches(st.get() + sf[g], sf[g + 1] - sf[g]);
        if (p.n_segments[g] != own.size()) bad++;
        segs += own.size();
        for (size_t k = 0; k < p.n_launches; k++) {
            const GroupSeg &s = p.launch(k)[g];
            if (k < own.size() ? !same(s, own[k].ext, int_phases(own[k]), own[k].n_int, own[k].hints) : !sits_out(s)) bad++;
        }
    }
    CHECK(bad == 0 && segs > 0, "%zu records differ from the groups' own plans", bad);
}

// ---- what the argument checks read from the arrays
static void check_arguments() {
    const Packed ok{{IE, I}, {}, {E}};
    CHECK(group_steps_check(3, ok.steps.get(), ok.first.get()) == 0, "good arrays");
    CHECK(group_steps_check(3, nullptr, ok.first.get()) == -2, "null steps with steps to read");
    const Packed nothing{{}, {}};
    CHECK(group_steps_check(2, nullptr, nothing.first.get()) == 0, "null steps with nothing to read");
    std::unique_ptr<uint32_t[]> f(new uint32_t[4]{0, 2, 1, 3});
    CHECK(group_steps_check(3, ok.steps.get(), f.get()) == -1, "step_first descends");
    f[0] = 1; f[2] = 2;
    CHECK(group_steps_check(3, ok.steps.get(), f.get()) == -1, "step_first does not start at 0");
    const Packed badb{{IE, I}, {4}};
    CHECK(group_steps_check(2, badb.steps.get(), badb.first.get()) == 3, "the bad byte's index, plus one");
}

int main() {
    check_plan_launches();
    check_equal();
    check_ragged();
    check_sizes();
    check_arguments();
    printf("group plan harness: %d failed checks\n", failures);
    return failures;
}
