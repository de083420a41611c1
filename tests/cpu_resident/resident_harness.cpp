// resident_harness.cpp — the host arithmetic of resident and lingering schedule launches (magics_amd/csrc/mgx_resident.h) on the
// CPU, as a stand-alone program meant to be built with -fsanitize=address,undefined (tests/test_resident_host.py): the plan bytes
// of a schedule cut into launches, parity and segment count through launches and posts, and from a recorded standing on after a take-back, the back-off after declined
// launches, the internal phases of a segment — each against values written out here by hand.  Prints one line per failed check and
// returns their number.
#include <cstdio>
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

// segment k of the test plans: an external iteration in front of every third one, 1 + (7 k mod 250) internal iterations (so the
// bytes differ from segment to segment and reach beyond 127)
static Launch segment(size_t k) { return Launch{k % 3 == 1 ? 3u : 0u, 1 + (int)((7 * k) % 250), (uint32_t)k}; }

// ---- the slice filler: plans of 1, 32, 33 and 71 segments cut into launches of 1 / 32 / 32 + 1 / 32 + 32 + 7
static void check_fill() {
    struct Case { size_t segments; int parts; int size[3]; };
    const Case cases[] = {{1, 1, {1, 0, 0}}, {32, 1, {32, 0, 0}}, {33, 2, {32, 1, 0}}, {71, 3, {32, 32, 7}}};
    for (const Case &c : cases) {
        std::vector<Launch> plan;
        for (size_t k = 0; k < c.segments; k++) plan.push_back(segment(k));
        int part = 0;
        for (size_t from = 0; from < plan.size(); from += 32, part++) {
            // exactly the plan's 32 bytes each, on the heap: a byte written beside them is the sanitizer's to report
            std::unique_ptr<uint8_t[]> ext(new uint8_t[32]), n_int(new uint8_t[32]);
            for (int k = 0; k < 32; k++) ext[k] = n_int[k] = 0xee;
            const int n = fill_segments(plan, from, ext.get(), n_int.get());
            CHECK(part < c.parts && n == c.size[part], "%zu segments, part %d: %d segments", c.segments, part, n);
            for (int k = 0; k < 32; k++) {
                const bool in = k < n;
                const uint8_t want_ext = in && (from + (size_t)k) % 3 == 1 ? 1 : 0;
                const uint8_t want_int = in ? (uint8_t)(1 + (7 * (from + (size_t)k)) % 250) : 0;
                CHECK(ext[k] == want_ext && n_int[k] == want_int, "%zu segments, part %d, byte %d: ext %u (%u) n_int %u (%u)", c.segments, part, k,
                      ext[k], want_ext, n_int[k], want_int);
            }
        }
        CHECK(part == c.parts, "%zu segments: %d parts, expected %d", c.segments, part, c.parts);
    }
    std::vector<Launch> none;  // (nothing to fill: no segments, all bytes zero, nothing read)
    uint8_t ext[32], n_int[32];
    CHECK(fill_segments(none, 0, ext, n_int) == 0 && ext[0] == 0 && n_int[31] == 0, "an empty plan");
}

// ---- parity and segment count: launch(11), post(11), post(1), a post(2) taken back and launched instead, launch(33) as 32 + 1
// (the take-back itself is an assignment of the recorded standing, Submitted::take_back in the library: what is checked here is
// the arithmetic on both sides of it)
static void check_standing() {
    auto closed_form = [](const Standing &s, int n) { return Standing{(s.cur + n) & 1, s.flag_base + (unsigned long long)n}; };
    auto same = [](const Standing &a, const Standing &b) { return a.cur == b.cur && a.flag_base == b.flag_base; };
    const Standing s0{1, 5};
    const Standing s1 = s0.after_launch(11);
    CHECK(s1.cur == 0 && s1.flag_base == 16 && same(s1, closed_form(s0, 11)), "launch(11): %d %llu", s1.cur, s1.flag_base);
    const Standing s2 = s1.after_post(11);  // (continues the last segment before it: ten more)
    CHECK(s2.cur == 0 && s2.flag_base == 26 && same(s2, closed_form(s1, 10)), "post(11): %d %llu", s2.cur, s2.flag_base);
    const Standing s3 = s2.after_post(1);
    CHECK(s3.cur == 0 && s3.flag_base == 26 && same(s3, closed_form(s2, 0)), "post(1): %d %llu", s3.cur, s3.flag_base);
    // a post that moves both, recorded as the host records it (where the world stood before), taken back, and run as a launch
    // of its own from there: the world ends where a launch of the same segments behind post(1) ends
    const Standing before = s3;
    Standing now = s3.after_post(2);
    CHECK(now.cur == 1 && now.flag_base == 27 && same(now, closed_form(before, 1)), "post(2): %d %llu", now.cur, now.flag_base);
    now = before;  // the take-back
    now = now.after_launch(2);
    CHECK(now.cur == 0 && now.flag_base == 28 && same(now, closed_form(s3, 2)), "post(2) taken back and launched: %d %llu", now.cur, now.flag_base);
    const Standing s4 = s3;
    const Standing s5 = s4.after_launch(32), s6 = s5.after_launch(1);
    CHECK(s5.cur == 0 && s5.flag_base == 58 && same(s5, closed_form(s4, 32)), "launch(32 of 33): %d %llu", s5.cur, s5.flag_base);
    CHECK(s6.cur == 1 && s6.flag_base == 59 && same(s6, closed_form(s4, 33)), "launch(1 of 33): %d %llu", s6.cur, s6.flag_base);
    const Standing top{1, ~0ull};  // the count runs modulo 2^64 (the ranks' flag_delta does too)
    CHECK(top.after_launch(3).cur == 0 && top.after_launch(3).flag_base == 2ull, "wrap-around");
}

// ---- the back-off: five declines in a row and a go; counting down; the cap
static void check_backoff() {
    Backoff b;
    CHECK(b.left == 0 && b.len == 0, "fresh");
    const int want[5] = {64, 128, 256, 512, 1024};
    for (int i = 0; i < 5; i++) {
        b.declined(11);
        CHECK(b.len == want[i] && b.left == want[i] + 11, "decline %d: len %d left %d", i + 1, b.len, b.left);
    }
    b.went_ahead();
    CHECK(b.len == 0, "go: len %d", b.len);
    b.declined(2);
    CHECK(b.len == 64 && b.left == 66, "a decline after a go: len %d left %d", b.len, b.left);
    for (int i = 0; i < 65; i++) b.external_iteration();
    CHECK(b.left == 1, "65 external iterations of 66: %d left", b.left);
    b.external_iteration();
    b.external_iteration();
    CHECK(b.left == 0, "never below zero: %d", b.left);
    for (int i = 0; i < 20; i++) b.declined(32);
    CHECK(b.len == 32768 && b.left == 32800, "the cap: len %d left %d", b.len, b.left);
}

static void check_phases_and_updates() {
    CHECK(int_phases(Launch{3u, 0, 0u}) == 0u, "n_int 0");
    CHECK(int_phases(Launch{0u, 1, 0u}) == 12u, "n_int 1");
    CHECK(int_phases(Launch{3u, 255, 0u}) == 12u, "n_int 255");
    const double rec[4] = {0, 0, 0, 0};
    RidingUpdates none, pinned, device;
    pinned.dev = pinned.host = rec;
    pinned.slot = 3;
    device.dev = rec;
    CHECK(!none.any() && none.postable() && none.slot == -1, "no updates");
    CHECK(pinned.any() && pinned.postable(), "records the host can read ride in a post");
    CHECK(device.any() && !device.postable(), "records in device memory do not");
}

int main() {
    check_fill();
    check_standing();
    check_backoff();
    check_phases_and_updates();
    printf("resident harness: %d failed checks\n", failures);
    return failures;
}
