// slots_due_check.cpp -- SlotSchedule's reason for a compaction (decide_due) and the tail squeeze's transition, against sm_slots.h alone
// (no HIP, no GPU).  Arguments: <tile> <cap> <max_new> <period> <bound> <stat frames> <stat slots> <frames enqueued>; then a script of
//   due      print decide_due() (0 none, 1 period, 2 forced) and decide_compact()
//   cull     cull_noted(false)            squeeze  squeezed_in_frame()            show  culls, maybe_garbage, keys_are_slots
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sm_slots.h"

using sm_slots::SlotSchedule;

int main(int argc, char **argv)
{
    if (argc < 9) return 2;
    auto num = [&](int i) { return std::strtoul(argv[i], nullptr, 10); };
    unsigned long long stat = 0;
    SlotSchedule s((uint32_t)num(1), (uint32_t)num(2), (uint32_t)num(3), (int)num(4), 0, &stat);
    s.state_pushed((uint32_t)num(8), 0);                       // appends enqueued
    stat = ((unsigned long long)num(6) << 32) | num(7);        // what the device last reported
    s.state_pulled((uint32_t)num(5), 0, false);                // the host's bound
    for (int i = 9; i < argc; ++i) {
        if (!std::strcmp(argv[i], "due")) std::printf("due %d %d\n", (int)s.decide_due(), s.decide_compact() ? 1 : 0);
        else if (!std::strcmp(argv[i], "cull")) { s.cull_noted(false); s.keys_drawn(true); }
        else if (!std::strcmp(argv[i], "squeeze")) { s.squeezed_in_frame(); s.keys_drawn(true); }
        else if (!std::strcmp(argv[i], "show")) std::printf("culls %d garbage %d keys %d\n", s.culls_since_compact(), s.maybe_garbage() ? 1 : 0, s.keys_are_slots() ? 1 : 0);
        else return 2;
    }
    return 0;
}
