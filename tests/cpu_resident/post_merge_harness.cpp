// post_merge_harness.cpp — the rule by which mgx_iterate merges back-to-back schedules into one post (post_merge_decide and
// linger_plan_fits, magics_amd/csrc/mgx_resident.h) on the CPU, as a stand-alone program meant to be built with
// -fsanitize=address,undefined (tests/test_post_merge_host.py).  Every expectation is written out here by hand.  Prints one line
// per failed check and returns their number.
#include <cstdio>
#include <string>

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

// the segments of a schedule given as its flattened phases ("IEIE..."): [E] I* each, as the library cuts them
static std::vector<Launch> plan_of(const std::string &phases) {
    std::vector<Launch> out;
    size_t i = 0;
    while (i < phases.size()) {
        Launch l{0u, 0, 0u};
        if (phases[i] == 'E') { l.ext = 3u; i++; }
        while (i < phases.size() && phases[i] == 'I') { l.n_int++; i++; }
        out.push_back(l);
    }
    return out;
}
static std::string times(const std::string &s, int n) {
    std::string out;
    for (int i = 0; i < n; i++) out += s;
    return out;
}
static const std::string TICK = times("IE", 10);  // the 10 / 10 schedule: I, nine E I, E — 11 segments; k of them merged: 10 k + 1
static const int OFF = POST_MERGE_OFF, AUTO = POST_MERGE_AUTO, ALWAYS = POST_MERGE_ALWAYS;
static const char *name(PostMerge d) { return d == PostMerge::SUBMIT ? "SUBMIT" : d == PostMerge::DEFER ? "DEFER" : "SUBMIT_RECORDED"; }

// decide for `fresh` issued behind `recorded` (phases; empty: nothing recorded); untaken: the THIRD post of the launch is outstanding
// and not taken (the launch is behind); otherwise it has been taken
static PostMerge decide_at(int mode, bool open, unsigned outstanding, bool taken, bool qualifies, const std::string &recorded, const std::string &fresh) {
    return post_merge_decide(mode, open, outstanding, taken, qualifies, !recorded.empty(), plan_of(fresh), plan_of(recorded + fresh));
}
static PostMerge decide(int mode, bool open, bool untaken, bool qualifies, const std::string &recorded, const std::string &fresh) {
    return decide_at(mode, open, 3u, !untaken, qualifies, recorded, fresh);
}

// ---- which post is outstanding: the first two of a launch are taken within a poll — mode 1 waits for them, as ever
static void check_outstanding() {
    for (unsigned k = 0; k <= 2; k++)
        for (int taken = 0; taken < 2; taken++) {
            CHECK(decide_at(AUTO, true, k, taken, true, "", TICK) == PostMerge::SUBMIT, "post %u of the launch outstanding: a post of its own", k);
            CHECK(decide_at(ALWAYS, true, k, taken, true, "", TICK) == PostMerge::DEFER, "mode 2 records behind post %u too", k);
        }
    for (unsigned k : {3u, 4u, 100u, 1000u}) {
        CHECK(decide_at(AUTO, true, k, false, true, "", TICK) == PostMerge::DEFER, "post %u untaken: the launch is behind", k);
        CHECK(decide_at(AUTO, true, k, true, true, "", TICK) == PostMerge::SUBMIT, "post %u taken", k);
        CHECK(decide_at(AUTO, true, k, false, true, times(TICK, 2), TICK) == PostMerge::DEFER && decide_at(AUTO, true, k, true, true, times(TICK, 2), TICK) == PostMerge::SUBMIT,
              "post %u, two recorded", k);
    }
    // a schedule without a single sweep is never recorded: what is recorded goes out, then it ends the launch as ever
    for (int mode : {OFF, AUTO, ALWAYS}) {
        CHECK(decide_at(mode, true, 3u, false, true, "", "") == PostMerge::SUBMIT, "no sweep, nothing recorded");
        CHECK(decide_at(mode, true, 3u, false, true, TICK, "") == PostMerge::SUBMIT_RECORDED, "no sweep behind a recorded tick");
    }
}

static void check_plans() {
    CHECK(plan_of(TICK).size() == 11, "one tick: %zu segments", plan_of(TICK).size());
    CHECK(plan_of(times(TICK, 2)).size() == 21 && plan_of(times(TICK, 3)).size() == 31 && plan_of(times(TICK, 4)).size() == 41, "merged ticks");
    CHECK(linger_plan_fits(plan_of(times(TICK, 3))) && !linger_plan_fits(plan_of(times(TICK, 4))), "three ticks fit a plan, four do not");
    CHECK(!linger_plan_fits(plan_of("")) && !linger_plan_fits(plan_of("EI")) && linger_plan_fits(plan_of("I")), "empty / opens external / one segment");
    CHECK(linger_plan_fits(plan_of(times("I", 255))) && !linger_plan_fits(plan_of(times("I", 256))), "a segment's iterations are one byte");
}

// ---- the post before: taken / untaken
static void check_taken() {
    CHECK(decide(AUTO, true, true, true, "", TICK) == PostMerge::DEFER, "untaken, nothing recorded");
    CHECK(decide(AUTO, true, false, true, "", TICK) == PostMerge::SUBMIT, "taken (or none outstanding), nothing recorded: a post of its own");
    CHECK(decide(AUTO, true, true, true, TICK, TICK) == PostMerge::DEFER, "untaken, one recorded");
    CHECK(decide(AUTO, true, false, true, TICK, TICK) == PostMerge::SUBMIT, "taken, one recorded: both as ONE plan");
    CHECK(decide(AUTO, true, false, true, times(TICK, 2), TICK) == PostMerge::SUBMIT, "taken, two recorded: three as ONE plan");
    CHECK(decide(ALWAYS, true, false, true, "", TICK) == PostMerge::DEFER && decide(ALWAYS, true, false, true, times(TICK, 2), TICK) == PostMerge::DEFER,
          "mode 2 records whatever was taken");
    for (int untaken = 0; untaken < 2; untaken++)
        for (int held = 0; held < 2; held++)
            CHECK(decide(OFF, true, untaken, true, held ? TICK : "", TICK) == PostMerge::SUBMIT, "mode 0 never records");
}

// ---- 10 + 10 + 10 segments fit, a fourth does not
static void check_three_ticks() {
    for (int mode : {AUTO, ALWAYS}) {
        CHECK(decide(mode, true, true, true, "", TICK) == PostMerge::DEFER, "first");
        CHECK(decide(mode, true, true, true, TICK, TICK) == PostMerge::DEFER, "second");
        CHECK(decide(mode, true, true, true, times(TICK, 2), TICK) == PostMerge::DEFER, "third");
        CHECK(decide(mode, true, true, true, times(TICK, 3), TICK) == PostMerge::SUBMIT_RECORDED, "the fourth does not fit: the three go out");
        CHECK(decide(mode, true, true, true, "", TICK) == PostMerge::DEFER, "... and the fourth is the first of the next plan");
    }
    CHECK(decide(AUTO, true, false, true, times(TICK, 3), TICK) == PostMerge::SUBMIT_RECORDED, "the fourth, previous post taken: still two plans");
    CHECK(decide(AUTO, false, false, true, times(TICK, 3), TICK) == PostMerge::SUBMIT_RECORDED, "the fourth, launch gone: two launches");
}

// ---- a 32-segment schedule alone; more than MAX_SEGS segments are never recorded
static void check_sizes() {
    const std::string s32 = "I" + times("EI", 31), s33 = "I" + times("EI", 32);
    CHECK(plan_of(s32).size() == 32 && plan_of(s33).size() == 33, "32 / 33 segments");
    CHECK(decide(AUTO, true, true, true, "", s32) == PostMerge::DEFER && decide(ALWAYS, true, false, true, "", s32) == PostMerge::DEFER, "32 segments alone are a plan");
    CHECK(decide(AUTO, true, true, true, "I", s32) == PostMerge::DEFER, "I ++ (I E I ...): the first segments fuse, still 32");
    CHECK(decide(AUTO, true, true, true, "IE", s32) == PostMerge::SUBMIT_RECORDED, "33 merged");
    for (int mode : {OFF, AUTO, ALWAYS})
        for (int open = 0; open < 2; open++)
            for (int untaken = 0; untaken < 2; untaken++)
                for (int q = 0; q < 2; q++) {
                    CHECK(decide(mode, open, untaken, q, "", s33) == PostMerge::SUBMIT, "33 segments, nothing recorded: submitted (as launches)");
                    CHECK(decide(mode, open, untaken, q, TICK, s33) == PostMerge::SUBMIT_RECORDED, "33 segments behind a recorded tick: never recorded");
                }
    CHECK(decide(AUTO, true, true, true, times("I", 200), times("I", 100)) == PostMerge::SUBMIT_RECORDED, "fused iterations beyond a byte");
}

// ---- a schedule that opens with an external iteration: it may follow in a merge, it cannot start a post
static void check_external_first() {
    const std::string ext = "EIEI";
    for (int mode : {OFF, AUTO, ALWAYS})
        for (int untaken = 0; untaken < 2; untaken++)
            CHECK(decide(mode, true, untaken, true, "", ext) == PostMerge::SUBMIT, "opens external, nothing recorded: not a post, never recorded");
    CHECK(decide(ALWAYS, true, true, true, TICK, ext) == PostMerge::DEFER && decide(ALWAYS, true, false, true, TICK, ext) == PostMerge::DEFER,
          "mode 2: it follows in a merge");
    CHECK(linger_plan_fits(plan_of(TICK + ext)), "... whose plan is a post");
    // automatic mode keeps apart what would not have been posted on its own: which schedules are posted and which launched then
    // does not depend on how far behind the device is (only how the posts are grouped does)
    CHECK(decide(AUTO, true, true, true, TICK, ext) == PostMerge::SUBMIT_RECORDED && decide(AUTO, true, false, true, TICK, ext) == PostMerge::SUBMIT_RECORDED,
          "mode 1: the recorded ones go out, it runs as the launch it would have been");
}

// ---- the launch ended meanwhile, or the world no longer takes posts: never defer
static void check_never_defer() {
    for (int mode : {OFF, AUTO, ALWAYS})
        for (int untaken = 0; untaken < 2; untaken++)
            for (int q = 0; q < 2; q++) {
                CHECK(decide(mode, false, untaken, q, "", TICK) == PostMerge::SUBMIT, "launch gone, nothing recorded");
                CHECK(decide(mode, false, untaken, q, times(TICK, 2), TICK) == PostMerge::SUBMIT, "launch gone: recorded ++ new as ONE launch");
            }
    for (int mode : {OFF, AUTO, ALWAYS})
        for (int untaken = 0; untaken < 2; untaken++) {
            CHECK(decide(mode, true, untaken, false, "", TICK) == PostMerge::SUBMIT, "world does not qualify");
            CHECK(decide(mode, true, untaken, false, TICK, TICK) == PostMerge::SUBMIT, "world does not qualify, one recorded");
        }
    // every combination: DEFER only with a launch that is open, a world that qualifies, merging on, and a merged plan that is a post
    const std::string shapes[] = {"", "I", TICK, times(TICK, 2), times(TICK, 3), "EIEI", "I" + times("EI", 31), times("I", 250)};
    for (int mode : {OFF, AUTO, ALWAYS})
        for (int bits = 0; bits < 8; bits++)
            for (const std::string &rec : shapes)
                for (const std::string &fresh : shapes) {
                    if (fresh.empty() || (!rec.empty() && !linger_plan_fits(plan_of(rec)))) continue;  // (what is recorded was a post)
                    const bool open = bits & 1, untaken = bits & 2, q = bits & 4;
                    const PostMerge d = decide(mode, open, untaken, q, rec, fresh);
                    const bool post = linger_plan_fits(plan_of(rec + fresh));
                    if (d == PostMerge::DEFER)
                        CHECK(open && q && mode != OFF && post && (mode == ALWAYS || untaken), "DEFER in mode %d, bits %d, %zu + %zu phases", mode, bits, rec.size(), fresh.size());
                    if (d == PostMerge::SUBMIT_RECORDED) CHECK(!rec.empty(), "SUBMIT_RECORDED with nothing recorded");
                    if (d == PostMerge::SUBMIT && !rec.empty()) CHECK(post, "%s of a merged plan that is no post", name(d));
                }
}

int main() {
    check_plans();
    check_taken();
    check_outstanding();
    check_three_ticks();
    check_sizes();
    check_external_first();
    check_never_defer();
    printf("post merge harness: %d failed checks\n", failures);
    return failures;
}
