// mgx_plan_pool.h — the bookkeeping of the global planner's request pool (mgx_plan_submit / _advance / _collect / _cancel,
// include/mgx.h): slots in blocks, the free list, ticket -> slot, the requests that have ended and the order they are handed out
// in.  Host arithmetic only: no HIP, no allocation of a slot's arrays (mgx_world_planner.inc does that, one block of slots at a
// time, and tells add_block) — so that it builds and runs on its own (tests/c_abi/plan_pool_fuzz.cpp).
// A world has two books, which differ in shape (slots_per_block x max_blocks): the riding requests', and mgx_plan_paths' own.
//
// A slot's life: FREE -> RUNNING (submit) -> ENDED (the device's completion log named its ticket) -> COOLING (collected) -> FREE.
// A cancelled request goes to COOLING from RUNNING or ENDED.  COOLING lasts until every slice enqueued when the slot was given
// up has completed (those launches may still list the slot): only then may another request's state be written into it.
#pragma once
#include <cstdint>
#include <set>
#include <tuple>
#include <unordered_map>
#include <utility>
#include <vector>

namespace mgx {

struct PlanPoolBook {
    enum : uint8_t { FREE = 0, RUNNING = 1, ENDED = 2, COOLING = 3 };
    struct Slot {
        uint64_t ticket = 0;
        uint64_t first_seq = 0;   // advances enqueued before the request was submitted: slice number = advance number - first_seq
        uint64_t free_after = 0;  // COOLING: the last advance that may still list the slot
        uint32_t slices = 0;      // ENDED: the slice it ended in
        uint8_t st = FREE;
    };
    uint32_t slots_per_block, max_blocks;  // the pool's shape (drop keeps it, reset sets another)
    std::vector<Slot> slots;
    std::vector<uint32_t> free_list;
    std::vector<uint32_t> cooling;
    std::unordered_map<uint64_t, uint32_t> by_ticket;          // RUNNING and ENDED requests
    std::set<std::tuple<uint32_t, uint64_t, uint32_t>> ended;  // (slices, ticket, slot): the order of mgx_plan_collect
    uint64_t next_ticket = 1;  // per world, never reused (drop keeps it)
    uint64_t seq = 0;          // advances enqueued
    uint64_t completed = 0;    // advances known to have completed
    uint32_t n_running = 0;
    bool list_dirty = true;    // the set of RUNNING slots changed since the active list was last written

    PlanPoolBook(uint32_t slots_per_block_, uint32_t max_blocks_) : slots_per_block(slots_per_block_), max_blocks(max_blocks_) {}
    uint32_t max_slots() const { return slots_per_block * max_blocks; }
    uint32_t pending() const { return (uint32_t)by_ticket.size(); }
    uint32_t blocks() const { return (uint32_t)(slots.size() / slots_per_block); }

    void add_block() {
        const uint32_t first = (uint32_t)slots.size();
        slots.resize(first + slots_per_block);
        for (uint32_t i = slots_per_block; i-- > 0;) free_list.push_back(first + i);  // (lowest index is taken first)
    }
    // a slot nothing in flight can touch, or -1: add a block first
    int take_slot() {
        if (free_list.empty()) return -1;
        const uint32_t s = free_list.back();
        free_list.pop_back();
        return (int)s;
    }
    void give_back(uint32_t s) { free_list.push_back(s); }  // (taken, then the submit was abandoned)
    uint64_t submit(uint32_t s) {
        Slot &q = slots[s];
        q.ticket = next_ticket++;
        q.first_seq = seq;
        q.slices = 0;
        q.st = RUNNING;
        by_ticket.emplace(q.ticket, s);
        n_running += 1;
        list_dirty = true;
        return q.ticket;
    }
    uint64_t advance() { return ++seq; }
    // an entry of the completion log.  Entries of requests cancelled meanwhile (their ticket is unknown) are dropped
    void finished(uint64_t ticket, uint32_t slices) {
        const auto it = by_ticket.find(ticket);
        if (it == by_ticket.end()) return;
        Slot &q = slots[it->second];
        if (q.st != RUNNING) return;
        q.st = ENDED;
        q.slices = slices;
        ended.emplace(slices, ticket, it->second);
        n_running -= 1;
        list_dirty = true;
    }
    bool next_done(uint64_t *ticket, uint32_t *slices, uint32_t *slot) const {
        if (ended.empty()) return false;
        std::tie(*slices, *ticket, *slot) = *ended.begin();
        return true;
    }
    void cool(uint32_t s) {
        slots[s].st = COOLING;
        slots[s].free_after = seq;
        cooling.push_back(s);
    }
    void pop_done() {
        const auto e = *ended.begin();
        ended.erase(ended.begin());
        by_ticket.erase(std::get<1>(e));
        cool(std::get<2>(e));
    }
    bool cancel(uint64_t ticket) {
        const auto it = by_ticket.find(ticket);
        if (it == by_ticket.end()) return false;
        const uint32_t s = it->second;
        Slot &q = slots[s];
        if (q.st == RUNNING) { n_running -= 1; list_dirty = true; }
        else ended.erase(std::make_tuple(q.slices, q.ticket, s));
        by_ticket.erase(it);
        cool(s);
        return true;
    }
    // every advance up to `upto` has completed
    void complete(uint64_t upto) {
        if (upto > completed) completed = upto;
        size_t keep = 0;
        for (size_t i = 0; i < cooling.size(); i++) {
            const uint32_t s = cooling[i];
            if (slots[s].free_after <= completed) { slots[s].st = FREE; free_list.push_back(s); }
            else cooling[keep++] = s;
        }
        cooling.resize(keep);
    }
    template <class F>
    void for_running(F f) const {
        for (uint32_t s = 0; s < (uint32_t)slots.size(); s++)
            if (slots[s].st == RUNNING) f(s, slots[s]);
    }
    // everything goes but the shape and the ticket counter (the caller frees the blocks); reset: and the shape is another
    void drop() { reset(slots_per_block, max_blocks); }
    void reset(uint32_t slots_per_block_, uint32_t max_blocks_) {
        const uint64_t t = next_ticket;
        *this = PlanPoolBook(slots_per_block_, max_blocks_);
        next_ticket = t;
    }
};

}  // namespace mgx
