"""The slot schedule (surfelmapping_amd/csrc/sm_slots.h: the host's bound on the occupied slots, which culls compact, the slot
estimate, the named transitions), without a GPU and without HIP: tests/cpp/slots_check.cpp is compiled against that header alone
and runs the scripts below.  The expected values are worked out by hand from the rules (DESIGN.md "Deferred compaction"), not
taken from the code."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "surfelmapping_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "slots_check.cpp")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("slots") / "slots_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I" + CSRC, "-o", exe, SRC])

    def run(script):
        r = subprocess.run([exe] + script.split(), capture_output=True, text=True, timeout=20)
        assert r.returncode == 0, (script, r.stdout, r.stderr)
        return r.stdout.splitlines()
    return run


def test_header_includes_no_hip():
    text = open(os.path.join(CSRC, "sm_slots.h")).read()
    assert "#include <hip" not in text and '#include "sm_ctx.h"' not in text and '#include "sm_device.h"' not in text


# capacity 1000, at most 100 new surfels per frame; `pushed F 0` sets the appends enqueued to F, `pulled B 0 0` the bound to B
def sched(period, wait_us=2000):
    return f"new 1024 1000 100 {period} {wait_us} "


@pytest.mark.parametrize("period", [0, 1])
def test_period_one_always_compacts(check, period):
    assert check(sched(period) + "pulled 300 0 0 decide cull 1 decide cull 1 append decide due") == ["decide 1"] * 3 + ["due 1"]


def test_every_fourth_cull_compacts(check):
    got = check(sched(4) + "pulled 300 0 0 decide cull 0 decide cull 0 decide cull 0 show decide cull 1 show decide")
    assert got == ["decide 0", "decide 0", "decide 0", "bound 300 culls 3 garbage 1 keys 0 stat 0 0 known 1 ahead 0",
                   "decide 1", "bound 300 culls 0 garbage 1 keys 0 stat 0 0 known 1 ahead 0", "decide 0"]


def test_capacity_rule(check):
    # (c) 500 + 2 * 100 = 700, + 100 <= 1000: fits, the period decides (first cull: no; fourth: yes)
    assert check(sched(4) + "pushed 12 0 pulled 950 0 0 stat 10 500 decide cull 0 cull 0 cull 0 decide") == ["decide 0", "decide 1"]
    # (d) 850 + 1 * 100 = 950 = the host's bound, + 100 > 1000 with the device one frame behind: compact
    assert check(sched(4) + "pushed 11 0 pulled 950 0 0 stat 10 850 decide") == ["decide 1"]
    # (e) the device three frames behind, but 850 + 2 * 100 > 1000 would not fit with it caught up either
    assert check(sched(4) + "pushed 13 0 pulled 1000 0 0 stat 10 850 decide") == ["decide 1"]
    # (f) 700 + 200 fits once the device has caught up: worth waiting for, and a wait of 0 us has expired at its first check
    assert check(sched(4, 0) + "pushed 13 0 pulled 1000 0 0 stat 10 700 decide") == ["decide 1"]
    # (g) ... and with 5 s to wait the device's next report (13, 750) arrives: 750 + 100 fits, the period (counter 0) says no
    assert check(sched(4, 5000000) + "pushed 13 0 pulled 1000 0 0 stat 10 700 later 30 13 750 decide show") == \
        ["decide 0", "bound 1000 culls 0 garbage 0 keys 0 stat 13 750 known 1 ahead 0"]
    # (h) a tag ahead of the host's count says nothing about the frames in between: only the host's bound counts
    assert check(sched(4) + "pushed 13 0 pulled 1000 0 0 stat 20 100 show decide") == \
        ["bound 1000 culls 0 garbage 0 keys 0 stat 20 100 known 0 ahead 0", "decide 1"]
    # the same tag with a bound that fits: the period decides
    assert check(sched(4) + "pushed 13 0 pulled 900 0 0 stat 20 100 decide") == ["decide 0"]


def test_sharded_stream_rules(check):
    # "the period is due" counts the cull about to be made; "the bound could overflow" uses the host's bound alone
    got = check(sched(3) + "pulled 900 0 0 due overflow cull 0 due cull 0 due overflow append overflow show pulled 850 0 0 overflow sharded due")
    assert got == ["due 0", "overflow 0", "due 0", "due 1", "overflow 0", "overflow 1",
                   "bound 1000 culls 2 garbage 1 keys 0 stat 0 0 known 1 ahead 1", "overflow 0", "due 0"]


def test_slot_estimate(check):
    est = "new 1024 1000000 100 4 2000 pushed 10 0 pulled 100000 0 0 "
    # 1. (8, 400) after the base (0, 0): rate min(400 / 8 + 1, 100) = 51, two appends ahead: 400 + 2 * 51
    # 2. (12, 900): fewer than 8 frames after the base (8, 400), the rate stands; nothing ahead
    # 3. (13, 100): the slots fell, the base restarts, the rate stands; 7 ahead clamped to the period 4: 100 + 4 * 51
    # 4. (21, 2100): 8 frames after (13, 100): rate min(2000 / 8 + 1, 100) = 100 -- seen once the host is 2 ahead again
    got = check(est + "stat 8 400 estimate append 2 stat 12 900 estimate append 8 stat 13 100 estimate stat 21 2100 estimate append 3 estimate show")
    assert got == ["estimate 502", "estimate 900", "estimate 304", "estimate 101000", "estimate 2300",
                   "bound 101300 culls 0 garbage 0 keys 0 stat 21 2100 known 1 ahead 2"]
    # never above the host's bound
    assert check("new 1024 1000000 100 4 2000 pushed 10 0 pulled 450 0 0 stat 8 400 estimate") == ["estimate 450"]
    # before the first rate is measured every enqueued frame may add anything: the bound
    assert check("new 1024 1000000 100 4 2000 pushed 3 0 pulled 5000 0 0 stat 1 40 estimate") == ["estimate 5000"]


def test_tiles_under_the_bound(check):
    for bound, tiles in ((0, 0), (1, 1), (1024, 1), (1025, 2), (0x7FFFFFFF, 1 << 21)):
        assert check(f"new 1024 2147483647 100 4 2000 pulled {bound} 0 0 tiles") == [f"tiles {tiles}"]
    assert check("new 1024 2147483647 100 4 2000 pulled 10 3000 1 tiles") == ["tiles 3"]       # a pending cull: its source still counts


def test_transitions_write_what_they_name(check):
    def show(script):
        (line,) = check(sched(4) + script + " show")
        return line
    dirty = "pulled 500 0 0 cull 0 cull 0 keys 1 "                     # two culls that only mark, the key map drawn as slots
    assert show(dirty) == "bound 500 culls 2 garbage 1 keys 1 stat 0 0 known 1 ahead 0"
    assert show(dirty + "cull 1") == "bound 500 culls 0 garbage 1 keys 1 stat 0 0 known 1 ahead 0"
    assert show(dirty + "keys 0") == "bound 500 culls 2 garbage 1 keys 0 stat 0 0 known 1 ahead 0"
    assert show(dirty + "compacted") == "bound 500 culls 0 garbage 0 keys 0 stat 0 0 known 1 ahead 0"
    assert show(dirty + "sharded") == "bound 500 culls 0 garbage 1 keys 0 stat 0 0 known 1 ahead 0"
    assert show(dirty + "dense") == "bound 500 culls 0 garbage 1 keys 1 stat 0 0 known 1 ahead 0"
    assert show(dirty + "discarded") == "bound 500 culls 2 garbage 0 keys 1 stat 0 0 known 1 ahead 0"
    assert show("pulled 500 0 0 dead") == "bound 500 culls 0 garbage 1 keys 0 stat 0 0 known 1 ahead 0"
    # an append: one more frame enqueued, at most 100 more slots, never above the capacity
    assert show(dirty + "append") == "bound 600 culls 2 garbage 1 keys 1 stat 0 0 known 1 ahead 1"
    assert show("pulled 950 0 0 append append") == "bound 1000 culls 0 garbage 0 keys 0 stat 0 0 known 1 ahead 2"
    # a pull replaces the bound; a push sets the statistic and the host's frame count to what it wrote
    assert show(dirty + "append pulled 420 0 0") == "bound 420 culls 2 garbage 1 keys 1 stat 0 0 known 1 ahead 1"
    assert show(dirty + "append pulled 420 800 1") == "bound 800 culls 2 garbage 1 keys 1 stat 0 0 known 1 ahead 1"
    assert show(dirty + "append pushed 7 420") == "bound 600 culls 2 garbage 1 keys 1 stat 7 420 known 1 ahead 0"
    assert check(sched(4) + "epoch epoch epoch") == ["epoch 1", "epoch 2", "epoch 3"]
