// mgx_resident.h — the arithmetic of the host's side of resident and lingering schedule launches (mgx_world_launch.inc drives
// them, mgx_world_types.h holds their state): a schedule's segments, their bytes in a launch's plan, where a world stands in its
// snapshot parity and segment count, the back-off after a declined launch, the prior updates that ride in a launch.  Free of HIP:
// compiles with a plain C++17 compiler (tests/cpu_resident/resident_harness.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mgx {

#ifndef __HIPCC__  // stand-alone: mgx_dev.h, which needs HIP, is not there — its values restated.  (In the library's build the assertion
                   // below reads mgx_dev.h's own constants: that is where a change there is caught; stand-alone it only checks these copies.)
constexpr uint32_t PH_EXT_FACTOR = 1u, PH_EXT_VARIABLE = 2u, PH_INT_FACTOR = 4u, PH_INT_VARIABLE = 8u;
constexpr uint32_t HINT_IR_DEAD = 1u, HINT_LATER_EXT_VARIABLE = 2u, HINT_LATER_INT_VARIABLE = 4u;
constexpr int MAX_SEGS = 32;
struct GroupSeg { uint32_t ext_mask, int_mask; int32_t n_int; uint32_t hints; };
#endif
static_assert((PH_INT_FACTOR | PH_INT_VARIABLE) == 12u && MAX_SEGS == 32, "the phases and the plan's size as mgx_dev.h has them");
static_assert((PH_EXT_FACTOR | PH_EXT_VARIABLE) == 3u && HINT_IR_DEAD == 1u && HINT_LATER_EXT_VARIABLE == 2u && HINT_LATER_INT_VARIABLE == 4u && sizeof(GroupSeg) == 16,
              "the external phases, the launch hints and a group's segment record as mgx_dev.h has them");

struct Launch { uint32_t ext; int n_int; uint32_t hints; };  // one [external iteration] internal* segment of a schedule
// the internal phases of a segment's launch: factor and variable sweeps together, or none
inline uint32_t int_phases(const Launch &l) { return l.n_int ? (PH_INT_FACTOR | PH_INT_VARIABLE) : 0; }

// The part of `plan` that starts at segment `from` as a launch's plan reads it (SegPlan and LingerPlan share the bytes): one byte
// per segment in ext[MAX_SEGS] and n_int[MAX_SEGS], zero behind the part.  Returns the part's segments (at most MAX_SEGS).
inline int fill_segments(const std::vector<Launch> &plan, size_t from, uint8_t *ext, uint8_t *n_int) {
    const int n = (int)std::min<size_t>((size_t)MAX_SEGS, plan.size() - std::min(from, plan.size()));
    for (int k = 0; k < MAX_SEGS; k++) {
        ext[k] = k < n && plan[from + (size_t)k].ext ? 1 : 0;
        n_int[k] = k < n ? (uint8_t)plan[from + (size_t)k].n_int : 0;
    }
    return n;
}

// The launches of a schedule: its steps' phases I / E flattened (robot.rs:1787-1860: internal first, then external, per step; bit 0
// of a step: internal, bit 1: external — MGX_STEP_*, include/mgx.h) and grouped into launches of the form [E] I* (one
// workgroup-resident pass each).
inline std::vector<Launch> plan_launches(const uint8_t *steps, uint32_t n) {
    std::vector<uint8_t> ph;
    for (uint32_t i = 0; i < n; i++) {
        if (steps[i] & 1u) ph.push_back('I');
        if (steps[i] & 2u) ph.push_back('E');
    }
    std::vector<Launch> out;
    size_t i = 0;
    while (i < ph.size()) {
        Launch l{0u, 0, 0u};
        if (ph[i] == 'E') { l.ext = PH_EXT_FACTOR | PH_EXT_VARIABLE; i++; }
        while (i < ph.size() && ph[i] == 'I') { l.n_int++; i++; }
        // the next launch of this call (if any) starts with an external phase: the inter-robot messages
        // this launch computes are recomputed before anything reads their HBM copy
        l.hints = (l.ext && i < ph.size()) ? HINT_IR_DEAD : 0u;
        // later launches of this call that run a variable sweep rewrite the belief images (nothing reads them in between)
        for (size_t j = i; j < ph.size(); j++) l.hints |= (ph[j] == 'E') ? HINT_LATER_EXT_VARIABLE : HINT_LATER_INT_VARIABLE;
        out.push_back(l);
    }
    return out;
}

// ---- one schedule per robot group (mgx_iterate_groups, include/mgx.h) --------------------------------------------------------------
// Group g runs steps[step_first[g] .. step_first[g + 1]).  Groups never exchange messages, so launch k of a MIXED call carries
// segment k of every group's own plan (plan_launches of its steps): one GroupSeg record per group and launch, which the robots'
// workgroups read in place of the kernel's scalars.  A group with fewer segments — or none: an empty range — sits the later
// launches out (an all-zero record).  The hints are promises about the SAME robot's next sweep: they are the ones the group's own
// plan carries, so each is true for the group or 0.
struct GroupPlan {
    uint32_t n_groups = 0;
    size_t n_launches = 0;            // the largest segment count over the groups
    std::vector<GroupSeg> recs;       // [n_launches][n_groups]
    std::vector<uint8_t> writes_snap; // [n_launches] some group runs an internal variable sweep: the launch writes snapshots
    std::vector<uint8_t> any_ext;     // [n_launches] some group runs an external phase
    std::vector<uint32_t> n_segments; // [n_groups] segments of the group's own plan
    const GroupSeg *launch(size_t k) const { return recs.data() + k * (size_t)n_groups; }
};
inline bool sits_out(const GroupSeg &s) { return s.ext_mask == 0u && !(s.int_mask != 0u && s.n_int > 0); }
inline GroupPlan plan_group_launches(uint32_t n_groups, const uint8_t *steps, const uint32_t *step_first) {
    GroupPlan gp;
    gp.n_groups = n_groups;
    gp.n_segments.assign(n_groups, 0u);
    std::vector<std::vector<Launch>> own((size_t)n_groups);
    for (uint32_t g = 0; g < n_groups; g++) {
        const uint32_t a = step_first[g], b = step_first[g + 1];
        if (b > a) own[g] = plan_launches(steps + a, b - a);
        gp.n_segments[g] = (uint32_t)own[g].size();
        gp.n_launches = std::max(gp.n_launches, own[g].size());
    }
    gp.recs.assign(gp.n_launches * (size_t)n_groups, GroupSeg{0u, 0u, 0, 0u});
    gp.writes_snap.assign(gp.n_launches, 0);
    gp.any_ext.assign(gp.n_launches, 0);
    for (uint32_t g = 0; g < n_groups; g++)
        for (size_t k = 0; k < own[g].size(); k++) {
            const Launch &l = own[g][k];
            gp.recs[k * (size_t)n_groups + g] = GroupSeg{l.ext, int_phases(l), l.n_int, l.hints};
            if (l.n_int > 0) gp.writes_snap[k] = 1;
            if (l.ext) gp.any_ext[k] = 1;
        }
    return gp;
}
// "All live groups equal": every group flagged in live[n_groups] has byte-equal steps — then the call IS the plain call with those
// steps.  *first: the first live group (whose steps those are); n_groups when no group is live (equal as well: nothing to run).
inline bool group_steps_equal(uint32_t n_groups, const uint8_t *steps, const uint32_t *step_first, const uint8_t *live, uint32_t *first) {
    uint32_t f = n_groups;
    for (uint32_t g = 0; g < n_groups; g++) {
        if (!live[g]) continue;
        if (f == n_groups) { f = g; continue; }
        const uint32_t n = step_first[g + 1] - step_first[g];
        if (n != step_first[f + 1] - step_first[f]) { *first = f; return false; }
        for (uint32_t i = 0; i < n; i++)
            if (steps[step_first[g] + i] != steps[step_first[f] + i]) { *first = f; return false; }
    }
    *first = f;
    return true;
}
// What the argument checks of the per-group calls read from the arrays alone: 0, or 1 + the index of the first step byte with a
// bit that is no MGX_STEP_*; -1: step_first does not ascend from 0; -2: there are steps to read and `steps` is null.
inline long long group_steps_check(uint32_t n_groups, const uint8_t *steps, const uint32_t *step_first) {
    if (step_first[0] != 0u) return -1;
    for (uint32_t g = 0; g < n_groups; g++)
        if (step_first[g + 1] < step_first[g]) return -1;
    if (!steps && step_first[n_groups]) return -2;
    for (uint32_t i = 0; i < step_first[n_groups]; i++)
        if (steps[i] & ~3u) return 1 + (long long)i;
    return 0;
}

// Where a world stands between launches: the parity of its snapshot buffers (DevWorld::cur) and its segment count (every
// progress word is below or at it).  A launch of n segments moves both by n; a post CONTINUES the last segment of the plan
// before it, so it moves them by n - 1.  Taking a launch or a post back is going back to where the world stood before it.
struct Standing {
    int cur = 0;
    unsigned long long flag_base = 0;
    Standing after_launch(int n) const { return {(cur + n) & 1, flag_base + (unsigned long long)n}; }
    Standing after_post(int n) const { return after_launch(n - 1); }
};

// After a declined launch the schedules skip the resident form for a while: `left` counts world-wide external iterations that
// ran launch by launch, `len` doubles with every decline in a row (64 .. 32768) and starts over with a launch that went ahead.
struct Backoff {
    int left = 0, len = 0;
    void declined(int segments) {  // (+ the declined schedule's own re-run)
        len = std::min(std::max(2 * len, 64), 32768);
        left = len + segments;
    }
    void external_iteration() { if (left > 0) left--; }
    void went_ahead() { len = 0; }
};

// A plan that can be POSTED into a launch that lingers: it fits the box's plan, and it opens with an internal iteration (a post
// CONTINUES the last segment of the plan before it).
inline bool linger_plan_fits(const std::vector<Launch> &plan) {
    if (plan.empty() || plan.size() > (size_t)MAX_SEGS || plan[0].ext) return false;
    for (const Launch &l : plan)
        if (l.n_int > 255) return false;
    return true;
}

// Merging back-to-back schedules into one post (mgx_iterate, mgx_set_post_merge).  While the launch that lingers is behind — the
// post before this call's has not been taken yet — the host would only spin; it records the schedule instead, and what is
// recorded rides with a later call's schedule as ONE plan: iterate(a); iterate(b) computes what iterate(a ++ b) computes, and
// the plan boundary between them (a trip of every belief image through HBM, three barriers, a poll) is never paid.
//   launch_open    a launch lingers, its census is confirmed and it has not ended (read once, never waited for)
//   outstanding    the place of the outstanding post among its launch's posts (1: the first behind the launch's own plan);
//                  0: no post is outstanding
//   taken          the launch has taken that post (read once, never waited for)
//   qualifies      the world can take a post at all (nothing dirty, nothing thawing, resident launches on, no back-off)
//   held           schedules are recorded already (their plan alone could be posted: that is why they were)
//   fresh          the plan of this call's schedule alone
//   merged         the plan of the recorded schedules ++ this call's (== fresh where nothing is recorded)
// SUBMIT: recorded ++ this call's schedule go out now, as one plan.  DEFER: this call's schedule is recorded behind the others.
// SUBMIT_RECORDED: what is recorded goes out alone (waiting as a post waits), then the call is decided again with nothing
// recorded.  A schedule is only ever recorded where it could be posted with what it is recorded behind, so a schedule of more
// than MAX_SEGS segments never is, and one that opens with an external iteration cannot be the first.  Mode AUTO records only
// schedules that would have been posted on their own as well (so what is posted and what is launched does not depend on how far
// behind the device happens to be: only how the posts are grouped does); mode ALWAYS lets a schedule that opens with an external
// iteration follow in a merge, and records whatever was taken — deterministic, for tests and diagnostics.
// Untaken BECAUSE THE LAUNCH IS BEHIND is what AUTO asks: the first two posts of a launch go into slots that are free whatever
// the workgroups are doing — the postman takes them within a poll — so finding one of them untaken says nothing about the
// device, and a schedule recorded behind it would only sit on the host (and, if the caller then went silent, miss the launch);
// from the third on, a post waits for every workgroup to have picked up the plan two before it.  So a launch and three posts
// go out singly, as ever.  A schedule without a single sweep is never recorded (it ends the launch, as ever).
enum PostMergeMode : int32_t { POST_MERGE_OFF = 0, POST_MERGE_AUTO = 1, POST_MERGE_ALWAYS = 2 };
enum class PostMerge { SUBMIT, DEFER, SUBMIT_RECORDED };
inline PostMerge post_merge_decide(int32_t mode, bool launch_open, unsigned outstanding, bool taken, bool qualifies, bool held,
                                   const std::vector<Launch> &fresh, const std::vector<Launch> &merged) {
    if (fresh.empty()) return held ? PostMerge::SUBMIT_RECORDED : PostMerge::SUBMIT;
    const bool post_untaken = outstanding > 2u && !taken;
    const bool joins = linger_plan_fits(merged) && (mode == POST_MERGE_ALWAYS || linger_plan_fits(fresh));
    if (held && !joins) return PostMerge::SUBMIT_RECORDED;
    const bool record = mode != POST_MERGE_OFF && launch_open && qualifies && joins && (mode == POST_MERGE_ALWAYS || post_untaken);
    return record ? PostMerge::DEFER : PostMerge::SUBMIT;
}

// mgx_tick's / mgx_mission_tick_end's prior updates that ride in a schedule's first launch: [R_local][4] f64 records
struct RidingUpdates {
    const double *dev = nullptr;   // as the kernel reads them (DevWorld::upd is written from here)
    const double *host = nullptr;  // the host's view of the same records; null: they live in device memory
    int slot = -1;                 // the pinned ring slot they sit in (released behind the launch that reads them); -1: none
    double max_speed = 0.0, delta_t = 0.0;
    bool any() const { return dev || host; }
    bool postable() const { return !dev || host; }  // records in device memory cannot ride in a post (the box is the host's)
};

}  // namespace mgx
