// sm_slots.h -- the host's side of the deferred compaction (DESIGN.md 4 "Deferred compaction"), once: how many slots of the
// model are occupied as far as the host knows, which culls compact, and what the compaction leaves behind (dead slots, a key map
// of slot numbers).  Host only: no HIP header, not sm_ctx.h (tests/cpp/slots_check.cpp compiles it with a plain C++ compiler).
// The host never waits for the device on the frame path, so everything here is a bound or an estimate made from
//   the bound     an upper bound of the device's slot count: exact after a synchronisation (state_pulled), one frame's worth of
//                 new surfels more for every append enqueued since (append_enqueued) -- after a hundred unsynchronised frames
//                 it is the capacity;
//   the statistic one pinned word the device writes after every cull and append: frames << 32 | occupied slots, read against
//                 the appends the host has enqueued.
#pragma once

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <thread>

namespace sm_slots {

// The statistic as read: fr, slots: frame tag and occupied slots at the device's last report; ahead: appends enqueued since that
// report -- known only while the tag is not ahead of the host's count (0 otherwise)
struct SlotStat { uint32_t fr, slots; bool ahead_known; uint32_t ahead; };

class SlotSchedule {
public:
    SlotSchedule() = default;
    // tile: slots per tile; cap: MAX_VERTICES; max_new: the most new surfels a frame can add (its candidate pixels);
    // stat: the pinned word (its owner keeps it alive)
    SlotSchedule(uint32_t tile, uint32_t cap, uint32_t max_new, int compact_period, long capacity_wait_us, unsigned long long *stat)
        : tile_(tile), cap_(cap), max_new_(max_new), period_(compact_period), wait_us_(capacity_wait_us), stat_(stat) {}

    // ---- what the host knows ----
    SlotStat read_stat() const
    {
        const unsigned long long v = __atomic_load_n(stat_, __ATOMIC_RELAXED);
        const uint32_t fr = (uint32_t)(v >> 32);
        return {fr, (uint32_t)v, frames_enq_ >= fr, frames_enq_ >= fr ? frames_enq_ - fr : 0u};
    }
    uint32_t bound() const { return bound_; }
    uint64_t tiles_of(uint64_t slots) const { return (slots + tile_ - 1) / tile_; }
    uint64_t tiles() const { return tiles_of(bound_); }                // tiles under the bound (grid sizing)
    bool maybe_garbage() const { return garbage_; }                    // dead slots may exist: a cull that only marks ran since the last physical compaction
    bool keys_are_slots() const { return keys_slots_; }                // the key map's ids are slot numbers, not positions among the live surfels
    int culls_since_compact() const { return culls_; }
    uint32_t next_cull_epoch() { return ++cull_epoch_; }               // the hand-off flags' value of the next compaction

    // Which culls compact.  The HOST decides (it must launch the matching kernels, and it must do so without waiting for the
    // device): every `compact_period`-th cull, and whenever dead slots could make the frame overflow the capacity (then the
    // result would differ from the reference's).
    bool period_due() const { return period_ <= 1 || culls_ + 1 >= period_; }
    // the host's bound alone (what every rank of a sharded stream knows) cannot rule out that the next frame overflows
    bool bound_may_overflow() const { return (uint64_t)bound_ + max_new_ > cap_; }
    // Why: `period` -- the period alone asked, and dead slots could not make the frame overflow; `forced` -- the capacity rule
    // asked (or every cull compacts: period <= 1).  A periodic compaction of a plain asynchronous stream may be a tail squeeze that
    // leaves dead slots behind; a forced one squeezes everything and appends densely.
    enum class Due { none, period, forced };
    bool decide_compact() const { return decide_due() != Due::none; }
    Due decide_due() const
    {
        if (period_ <= 1) return Due::forced;
        // Capacity: a cull that only marks the dead must not be able to make the frame overflow because of them.
        // bound = slots at the last device update + one frame's worth of new surfels for every append enqueued since.
        // When the host has run far ahead of the device the bound is loose; rather than compacting for nothing it then
        // lets the device catch up (the queue still holds every frame in between, so the GPU stays busy).
        // (This is the one place where an "enqueue only" call may wait, and only within one frame's worth of the capacity:
        //  at most capacity_wait_us, default 2000 us, then it compacts instead.)
        const auto t_start = std::chrono::steady_clock::now();
        for (uint32_t spins = 0;; ++spins) {
            const SlotStat st = read_stat();
            uint64_t bound = bound_;
            if (st.ahead_known) bound = std::min<uint64_t>(bound, (uint64_t)st.slots + (uint64_t)st.ahead * max_new_);
            if (bound + max_new_ <= cap_) break;                           // fits even if every candidate pixel is new
            if (st.ahead <= 1u) return Due::forced;                        // the bound is (nearly) exact: compact
            if ((uint64_t)st.slots + 2ull * max_new_ > cap_) return Due::forced;  // would not fit with the device caught up either
            if ((spins & 63u) == 63u &&
                std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_start).count() > wait_us_)
                return Due::forced;                                        // the device is further behind than we are willing to wait for
            std::this_thread::yield();
        }
        return period_due() ? Due::period : Due::none;
    }

    // An ESTIMATE of the occupied slots (the surfel pass's grid policy): the statistic plus the measured growth for every append
    // enqueued since, never above the bound.
    uint64_t estimate_slots()
    {
        uint64_t est = bound_;
        const SlotStat st = read_stat();
        // growth per frame as the device has reported it (between two reports at least 8 frames apart), at most a frame's candidates
        if (st.fr < est_fr0_ || st.slots < est_slots0_) { est_fr0_ = st.fr; est_slots0_ = st.slots; }      // (a compaction, a reset: the rate stands)
        else if (st.fr >= est_fr0_ + 8u) {
            est_rate_ = std::min<uint32_t>((st.slots - est_slots0_) / (st.fr - est_fr0_) + 1u, max_new_);
            est_fr0_ = st.fr; est_slots0_ = st.slots;
        }
        // (a compaction comes at least every `compact_period` frames: the slots do not grow for longer than that)
        const uint32_t ahead = std::min<uint32_t>(st.ahead, (uint32_t)std::max(period_, 1));
        if (st.ahead_known) est = std::min<uint64_t>(est, (uint64_t)st.slots + (uint64_t)ahead * est_rate_);
        return est;
    }

    // ---- transitions: every write of the schedule is one of these ----
    // a cull was enqueued
    void cull_noted(bool compacted)
    {
        if (compacted) { culls_ = 0; }
        else { culls_++; garbage_ = true; }
    }
    // a squeeze was enqueued between the two launches of a frame, ahead of its cull (tail squeeze): the period restarts; dead slots
    // may remain below the squeeze's boundary and that frame's cull marks more, and its splat still draws slot numbers
    void squeezed_in_frame() { culls_ = 0; garbage_ = true; }
    // an append was enqueued (the device bumps the statistic's frame tag with it): at most max_new more slots
    void append_enqueued()
    {
        frames_enq_++;
        bound_ = (uint32_t)std::min<uint64_t>((uint64_t)bound_ + max_new_, cap_);
    }
    // the host has read the device's state (device idle): the bound is exact -- the slots, or the not yet applied cull's source
    void state_pulled(uint32_t count, uint32_t cull_n, bool pending_cull) { bound_ = std::max(count, cull_n * (pending_cull ? 1u : 0u)); }
    // the host has written the device's state (device idle): the statistic says what the device would have
    void state_pushed(uint32_t stat_frames, uint32_t count)
    {
        __atomic_store_n(stat_, ((unsigned long long)stat_frames << 32) | (unsigned long long)count, __ATOMIC_RELAXED);
        frames_enq_ = stat_frames;
    }
    // alive bits were cleared outside a cull (a retirement)
    void dead_slots_made() { garbage_ = true; }
    // a frame's splat drew the key map: slot numbers iff its cull moved nothing
    void keys_drawn(bool as_slots) { keys_slots_ = as_slots; }
    // The four compactions outside a frame differ in what they reset; each difference is kept:
    // ensure_compact's own: no dead slots, and the key map translated to positions
    void compacted_outside_frame() { garbage_ = false; culls_ = 0; keys_slots_ = false; }
    // a sharded stream's: garbage_ stays -- a rank always holds the other ranks' slots as dead ones and never asks (ensure_compact
    // compacts a sharded stream unconditionally)
    void compacted_sharded() { culls_ = 0; keys_slots_ = false; }
    // publish_dense's: the period restarts and nothing else -- its callers have compacted (or refilled the alive bits) before it; kept as found
    void published_dense() { culls_ = 0; }
    // the alive bits were refilled: nothing is dead.  The period and the key map are left to the publish_dense that follows; kept as found
    void model_discarded() { garbage_ = false; }

private:
    uint32_t tile_ = 1, cap_ = 0, max_new_ = 0;
    int period_ = 1;
    long wait_us_ = 0;
    unsigned long long *stat_ = nullptr;
    uint32_t bound_ = 0;               // host upper bound of the device-side count
    uint32_t frames_enq_ = 0;          // appends enqueued so far (compared with the statistic's tag)
    int culls_ = 0;                    // culls since the last compaction (the period's counter)
    bool garbage_ = false, keys_slots_ = false;
    uint32_t cull_epoch_ = 0;
    uint32_t est_fr0_ = 0, est_slots0_ = 0, est_rate_ = 0xFFFFFFFFu;   // the estimate's base report and the growth per frame measured from it
};

}  // namespace sm_slots
