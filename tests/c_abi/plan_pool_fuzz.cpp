// The bookkeeping of the global planner's request pool (magics_amd/csrc/mgx_plan_pool.h) on its own, without HIP: 10 000 random
// submit / advance / complete / collect / cancel steps against a plain model of what the C ABI promises.  A "device" is played
// by this program: a launch is the list of slots running when it was enqueued, it completes later, and a request ends in the
// slice the model drew for it.  The same walk runs over two shapes of pool: 256 blocks of 16 slots (the pool whose requests ride
// the stream) and one block of 5 slots (the kind mgx_plan_paths builds for a call; here it is full most of the time, and a submit
// finds every slot pending or cooling).  Built with -fsanitize=address,undefined by tests/test_planner_slices.py; exit status 0
// and a line "plan pool ok" per shape mean every check held.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "../../magics_amd/csrc/mgx_plan_pool.h"

using mgx::PlanPoolBook;

#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::fprintf(stderr, "line %d: %s (step %d)\n", __LINE__, #cond, step); \
            return 1;                                                           \
        }                                                                       \
    } while (0)

struct Launch {
    uint64_t seq;
    std::vector<std::pair<uint32_t, uint64_t>> list;  // (slot, ticket) as the active list held them
};
struct Model {
    uint32_t need;       // the slice it ends in
    uint64_t first_seq;
    bool ended = false;  // the log entry has been delivered
    uint32_t slot;
};

static int walk(const int steps, const uint64_t seed, const uint32_t slots_per_block, const uint32_t max_blocks) {
    std::mt19937_64 rng(seed);
    PlanPoolBook book(slots_per_block, max_blocks);
    const uint32_t most = std::min(200u, book.max_slots());
    std::map<uint64_t, Model> live;      // submitted, neither collected nor cancelled
    std::set<uint64_t> gone;             // collected or cancelled
    std::deque<Launch> flight;           // enqueued, not completed
    std::vector<std::pair<uint32_t, uint64_t>> list;  // the active list as last written
    uint64_t last_ticket = 0, collected = 0, cancelled = 0, reused = 0;
    std::set<uint32_t> ever_used;
    int step = 0;
    for (; step < steps; step++) {
        const unsigned op = (unsigned)(rng() % 100);
        if (op < 30) {  // submit 1..5
            const unsigned n = 1 + (unsigned)(rng() % 5);
            for (unsigned i = 0; i < n && book.pending() < most; i++) {
                int s = book.take_slot();
                if (s < 0 && book.blocks() == book.max_blocks) {  // every slot is pending or cooling: the submit is refused
                    CHECK(book.cooling.size() + live.size() == book.slots.size() && !book.cooling.empty());
                    break;
                }
                if (s < 0) {
                    book.add_block();
                    CHECK(book.slots.size() == (size_t)book.blocks() * slots_per_block);
                    s = book.take_slot();
                }
                CHECK(s >= 0 && (size_t)s < book.slots.size());
                for (const Launch &l : flight)  // nothing in flight may still list the slot
                    for (const auto &e : l.list) CHECK(e.first != (uint32_t)s);
                for (const auto &m : live) CHECK(m.second.slot != (uint32_t)s);
                if (!ever_used.insert((uint32_t)s).second) reused++;
                const uint64_t t = book.submit((uint32_t)s);
                CHECK(t == last_ticket + 1);
                last_ticket = t;
                Model m;
                m.need = 1 + (uint32_t)(rng() % 6);
                m.first_seq = book.seq;
                m.slot = (uint32_t)s;
                live.emplace(t, m);
            }
        } else if (op < 60) {  // advance
            if (book.n_running == 0) continue;
            if (book.list_dirty) {
                list.clear();
                book.for_running([&](uint32_t s, const PlanPoolBook::Slot &q) { list.emplace_back(s, q.ticket); });
                book.list_dirty = false;
                CHECK(list.size() == book.n_running);
            }
            Launch l;
            l.seq = book.advance();
            l.list = list;
            flight.push_back(l);
        } else if (op < 80) {  // the oldest launch completes: its log entries arrive, then the event
            if (flight.empty()) continue;
            const Launch l = flight.front();
            flight.pop_front();
            for (const auto &e : l.list) {
                const auto it = live.find(e.second);
                if (it == live.end()) {  // cancelled meanwhile: the device may still report it
                    if (rng() % 2) book.finished(e.second, 1);
                    continue;
                }
                Model &m = it->second;
                if (!m.ended && l.seq - m.first_seq == m.need) {
                    book.finished(e.second, m.need);
                    m.ended = true;
                }
            }
            book.complete(l.seq);
        } else if (op < 92) {  // collect up to 3
            unsigned room = 1 + (unsigned)(rng() % 3);
            uint64_t ticket = 0, before_t = 0;
            uint32_t slices = 0, slot = 0, before_s = 0;
            while (room-- && book.next_done(&ticket, &slices, &slot)) {
                const auto it = live.find(ticket);
                CHECK(it != live.end() && it->second.ended && it->second.need == slices && it->second.slot == slot);
                CHECK(std::make_pair(before_s, before_t) < std::make_pair(slices, ticket));
                for (const auto &m : live)  // nothing that has ended comes before it
                    if (m.second.ended) CHECK(std::make_pair(slices, ticket) <= std::make_pair(m.second.need, m.first));
                before_s = slices;
                before_t = ticket;
                book.pop_done();
                live.erase(it);
                CHECK(gone.insert(ticket).second);
                collected++;
            }
        } else {  // cancel: a live ticket, or one that is gone or was never given
            if (!live.empty() && rng() % 4) {
                auto it = live.begin();
                std::advance(it, (long)(rng() % live.size()));
                const uint64_t t = it->first;
                CHECK(book.cancel(t));
                live.erase(it);
                CHECK(gone.insert(t).second);
                CHECK(!book.cancel(t));
                cancelled++;
            } else {
                CHECK(!book.cancel(last_ticket + 1 + rng() % 7));
                if (!gone.empty()) CHECK(!book.cancel(*gone.begin()));
            }
        }
        CHECK(book.pending() == live.size());
        uint32_t running = 0;
        for (const auto &m : live) running += m.second.ended ? 0 : 1;
        CHECK(book.n_running == running);
        CHECK(book.ended.size() == live.size() - running);
        CHECK(book.free_list.size() + book.cooling.size() + live.size() == book.slots.size());
    }
    CHECK(book.slots.size() <= book.max_slots());
    // drop keeps the ticket counter and the shape; reset sets another shape
    book.drop();
    CHECK(book.pending() == 0 && book.slots.empty() && book.next_ticket == last_ticket + 1);
    CHECK(book.slots_per_block == slots_per_block && book.max_blocks == max_blocks);
    book.reset(slots_per_block + 1, 1);
    CHECK(book.max_slots() == slots_per_block + 1 && book.slots.empty() && book.next_ticket == last_ticket + 1);
    CHECK(collected > 100 && cancelled > 100 && reused > 100);
    std::printf("plan pool ok, %u x %u slots: %d steps, %llu tickets, %llu collected, %llu cancelled, %llu slots taken again\n", max_blocks,
                slots_per_block, steps, (unsigned long long)last_ticket, (unsigned long long)collected, (unsigned long long)cancelled, (unsigned long long)reused);
    return 0;
}

int main(int argc, char **argv) {
    const int steps = argc > 1 ? std::atoi(argv[1]) : 10000;
    const uint64_t seed = argc > 2 ? (uint64_t)std::atoll(argv[2]) : 12345u;
    const int rc = walk(steps, seed, 16, 256);
    return rc ? rc : walk(steps, seed, 5, 1);
}
