// slots_check.cpp -- drives surfelmapping_amd/csrc/sm_slots.h alone for tests/test_slots_cpu.py: no HIP header, any C++17
// compiler.  The arguments are a script run from left to right against one SlotSchedule and one statistic word; every command
// that asks something prints one line.
//   new <tile> <cap> <max_new> <period> <wait_us>     a fresh schedule (the statistic word zeroed)
//   stat <fr> <slots>                                 the device reports: the statistic word is stored
//   later <ms> <fr> <slots>                           ... from a second thread, <ms> after this command (joined at the end)
//   pulled <count> <cull_n> <pending>   pushed <stat_frames> <count>   append [n]   cull <compacted>   dead   keys <as_slots>
//   compacted   sharded   dense   discarded           the transitions
//   decide | due | overflow | estimate | tiles | epoch   print "<command> <value>"
//   show                                              print "bound B culls C garbage G keys K stat FR SLOTS known A ahead N"
#include "sm_slots.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using sm_slots::SlotSchedule;

static unsigned long long pack(const char *fr, const char *slots)
{
    return (strtoull(fr, nullptr, 10) << 32) | strtoull(slots, nullptr, 10);
}

int main(int argc, char **argv)
{
    static unsigned long long stat = 0;
    SlotSchedule s;
    std::vector<std::thread> later;
    auto num = [&](int i) { return i < argc ? strtoll(argv[i], nullptr, 10) : 0ll; };
    int rc = 0;
    for (int i = 1; i < argc && !rc; ++i) {
        const char *c = argv[i];
        auto is = [c](const char *name) { return strcmp(c, name) == 0; };
        if (is("new") && i + 5 < argc) {
            __atomic_store_n(&stat, 0ull, __ATOMIC_RELAXED);
            s = SlotSchedule((uint32_t)num(i + 1), (uint32_t)num(i + 2), (uint32_t)num(i + 3), (int)num(i + 4), (long)num(i + 5), &stat);
            i += 5;
        } else if (is("stat") && i + 2 < argc) {
            __atomic_store_n(&stat, pack(argv[i + 1], argv[i + 2]), __ATOMIC_RELAXED);
            i += 2;
        } else if (is("later") && i + 3 < argc) {
            const long long ms = num(i + 1);
            const unsigned long long v = pack(argv[i + 2], argv[i + 3]);
            later.emplace_back([ms, v] {
                std::this_thread::sleep_for(std::chrono::milliseconds(ms));
                __atomic_store_n(&stat, v, __ATOMIC_RELAXED);
            });
            i += 3;
        } else if (is("pulled") && i + 3 < argc) { s.state_pulled((uint32_t)num(i + 1), (uint32_t)num(i + 2), num(i + 3) != 0); i += 3; }
        else if (is("pushed") && i + 2 < argc) { s.state_pushed((uint32_t)num(i + 1), (uint32_t)num(i + 2)); i += 2; }
        else if (is("append")) {
            long long n = 1;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') n = num(++i);
            while (n-- > 0) s.append_enqueued();
        }
        else if (is("cull") && i + 1 < argc) { s.cull_noted(num(i + 1) != 0); i += 1; }
        else if (is("dead")) s.dead_slots_made();
        else if (is("keys") && i + 1 < argc) { s.keys_drawn(num(i + 1) != 0); i += 1; }
        else if (is("compacted")) s.compacted_outside_frame();
        else if (is("sharded")) s.compacted_sharded();
        else if (is("dense")) s.published_dense();
        else if (is("discarded")) s.model_discarded();
        else if (is("decide")) printf("decide %d\n", s.decide_compact() ? 1 : 0);
        else if (is("due")) printf("due %d\n", s.period_due() ? 1 : 0);
        else if (is("overflow")) printf("overflow %d\n", s.bound_may_overflow() ? 1 : 0);
        else if (is("estimate")) printf("estimate %llu\n", (unsigned long long)s.estimate_slots());
        else if (is("tiles")) printf("tiles %llu\n", (unsigned long long)s.tiles());
        else if (is("epoch")) printf("epoch %u\n", s.next_cull_epoch());
        else if (is("show")) {
            const sm_slots::SlotStat st = s.read_stat();
            printf("bound %u culls %d garbage %d keys %d stat %u %u known %d ahead %u\n", s.bound(), s.culls_since_compact(),
                   s.maybe_garbage() ? 1 : 0, s.keys_are_slots() ? 1 : 0, st.fr, st.slots, st.ahead_known ? 1 : 0, st.ahead);
        } else {
            fprintf(stderr, "slots_check: bad command '%s'\n", c);
            rc = 2;
        }
    }
    for (auto &t : later) t.join();
    return rc;
}
