// radii_harness.cpp — the per-segment thresholds of a grouped world's neighbour search (group_tables + group_thresholds,
// magics_amd/csrc/mgx_search.h) on the CPU, as a stand-alone program meant to be built with -fsanitize=address,undefined
// (tests/test_groups_radii_host.py): one threshold per SEGMENT, from the radius of the segment's group — a group nobody of the
// query is in has no segment and shifts nobody's; a threshold is squared_threshold of its radius; the table says whether it
// changed.  Prints one line per failed check and returns their number.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
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

static bool same_bits(float a, float b) { return memcmp(&a, &b, sizeof(float)) == 0; }

// squared_threshold against its definition, by brute force around radius^2: the largest f32 s whose f32 root does not exceed radius
static void check_threshold(float radius) {
    const float t = squared_threshold(radius);
    auto root = [](float s) { return (float)std::sqrt((double)s); };
    CHECK(!(root(t) > radius), "radius %.9g: the threshold's root %.9g exceeds it", radius, root(t));
    const float up = std::nextafter(t, std::numeric_limits<float>::infinity());
    CHECK(std::isinf(up) || root(up) > radius, "radius %.9g: a larger s (%.9g) is still in range", radius, up);
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    for (float r : {5.0f, std::nextafter(5.0f, 0.0f), 0.5f, 0.0f, 1e-30f, 3e19f, 20.f, 40.f, 60.f, 80.f, 1.0f / 3.0f}) check_threshold(r);
    const float t5 = squared_threshold(5.0f);  // (a little above 25: the largest s whose root still ROUNDS to 5)
    CHECK(t5 >= 25.0f && t5 < 25.00001f, "5 -> %.9g", t5);
    CHECK(squared_threshold(std::nextafter(5.0f, 0.0f)) < 25.0f, "the float below 5 keeps a pair at exactly 5 out");
    CHECK(squared_threshold(0.0f) == 0.0f && squared_threshold(-1.0f) < 0.0f && squared_threshold(-inf) < 0.0f, "zero and negative radii");
    CHECK(std::isnan(squared_threshold(nan)) && squared_threshold(inf) == inf, "NaN and inf radii");

    // groups 1, 3, 4, 6 present; 0, 2 and 5 absent: thresholds by SEGMENT, from the radii by GROUP
    const std::vector<uint32_t> group = {4, 1, 6, 3, 1, 4, 4, 6};
    const std::vector<float> radii = {100.f, 5.0f, 200.f, std::nextafter(5.0f, 0.0f), 0.0f, 300.f, nan};
    GroupTables t;
    CHECK(group_tables(group.data(), (int)group.size(), t), "tables");
    CHECK(t.thr.empty() && t.seg_group.size() == 4, "group_tables leaves the thresholds to group_thresholds; %zu segments", t.seg_group.size());
    CHECK(t.seg_group[0] == 1 && t.seg_group[1] == 3 && t.seg_group[2] == 4 && t.seg_group[3] == 6, "the segments' groups");
    CHECK(group_thresholds(t, radii.data(), radii.size(), 7.f), "the first thresholds are new");
    CHECK(t.thr.size() == 4, "%zu thresholds", t.thr.size());
    if (t.thr.size() == 4) {
        CHECK(same_bits(t.thr[0], squared_threshold(radii[1])) && same_bits(t.thr[1], squared_threshold(radii[3])) &&
                  same_bits(t.thr[2], squared_threshold(radii[4])) && same_bits(t.thr[3], squared_threshold(radii[6])),
              "an absent group shifted its neighbours' radii: %.9g %.9g %.9g %.9g", t.thr[0], t.thr[1], t.thr[2], t.thr[3]);
        CHECK(t.thr[0] == t5 && t.thr[1] < 25.0f && t.thr[2] == 0.0f && std::isnan(t.thr[3]), "the values");
    }
    CHECK(t.off_thr() == t.words() && t.words_with_thr() == t.words() + 4 && t.words() == t.members.size() + t.seg.size() + t.wg.size(), "offsets");
    // the same radii again (a NaN among them): nothing to upload; an ABSENT group's radius changes: nothing either; a present one's: new
    CHECK(!group_thresholds(t, radii.data(), radii.size(), 7.f), "the same radii are not new");
    std::vector<float> r2 = radii;
    r2[0] = 1.f; r2[2] = 2.f; r2[5] = 3.f;
    CHECK(!group_thresholds(t, r2.data(), r2.size(), 9.f), "radii of groups without a segment do not matter");
    r2[4] = 0.5f;
    CHECK(group_thresholds(t, r2.data(), r2.size(), 9.f) && t.thr.size() == 4 && same_bits(t.thr[2], squared_threshold(0.5f)) && t.thr[0] == t5, "one radius changed");
    // no radii: the scalar for every segment; radii that end before a segment's group: the scalar for that segment
    CHECK(group_thresholds(t, nullptr, 0, 5.0f) && t.thr[0] == t5 && t.thr[1] == t5 && t.thr[2] == t5 && t.thr[3] == t5, "one radius for all");
    CHECK(!group_thresholds(t, nullptr, 0, 5.0f), "... twice");
    CHECK(group_thresholds(t, radii.data(), 4, 2.0f) && same_bits(t.thr[2], squared_threshold(2.0f)) && same_bits(t.thr[3], squared_threshold(2.0f)) &&
              t.thr[0] == t5, "groups beyond the radii take the scalar");
    // robots leave: the tables are built again and hold no thresholds until they are made again — also with the radii they had
    const std::vector<uint32_t> fewer = {4, 6, 4};
    CHECK(group_tables(fewer.data(), (int)fewer.size(), t) && t.thr.empty() && t.seg_group.size() == 2, "new tables");
    CHECK(group_thresholds(t, radii.data(), radii.size(), 7.f) && t.thr.size() == 2 && t.thr[0] == 0.0f && std::isnan(t.thr[1]), "new tables, new thresholds");
    // an empty query
    CHECK(group_tables(nullptr, 0, t) && t.n_segments() == 0, "an empty query");
    CHECK(group_thresholds(t, radii.data(), radii.size(), 7.f) || t.thr.empty(), "no segments, no thresholds");
    CHECK(t.thr.empty() && t.words_with_thr() == t.words(), "no segments, no thresholds");
    printf("radii harness: %d failed checks\n", failures);
    return failures;
}
