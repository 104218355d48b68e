"""SlotSchedule::decide_due -- WHY a cull compacts -- and the tail squeeze's transition (surfelmapping_amd/csrc/sm_slots.h), without a
GPU: tests/cpp/slots_due_check.cpp is compiled against the header alone.  A compaction only the period asked for may be a tail
squeeze that leaves dead slots behind (DESIGN.md 4 "Tail squeeze"); one the capacity rule asked for must not.  Expected values are
worked out from the rules: capacity 1000, at most 100 new surfels per frame."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "surfelmapping_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "slots_due_check.cpp")
NONE, PERIOD, FORCED = 0, 1, 2


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("slots_due") / "slots_due_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I" + CSRC, "-o", exe, SRC])

    def run(period, bound, stat_frames, stat_slots, enqueued, script):
        r = subprocess.run([exe, "1024", "1000", "100", str(period), str(bound), str(stat_frames), str(stat_slots), str(enqueued)] + script.split(),
                           capture_output=True, text=True, timeout=20)
        assert r.returncode == 0, (script, r.stdout, r.stderr)
        return r.stdout.splitlines()
    return run


def test_the_period_alone_is_due_period(check):
    # bound 300 + 100 <= 1000: the capacity rule is silent; the third cull of period 3 is due
    assert check(3, 300, 0, 300, 0, "due cull due cull due") == [f"due {NONE} 0", f"due {NONE} 0", f"due {PERIOD} 1"]


def test_every_cull_compacting_is_forced(check):
    assert check(1, 300, 0, 300, 0, "due") == [f"due {FORCED} 1"]


def test_the_capacity_rule_is_forced_whatever_the_period_says(check):
    # bound 950 + 100 > 1000 with the device caught up (no append outstanding): forced, on the first cull and on the period's
    assert check(3, 950, 5, 950, 5, "due cull cull due") == [f"due {FORCED} 1", f"due {FORCED} 1"]


def test_a_squeeze_restarts_the_period_and_leaves_garbage_and_slot_keys(check):
    got = check(3, 300, 0, 300, 0, "cull cull show due squeeze show due cull cull due")
    assert got == ["culls 2 garbage 1 keys 1", f"due {PERIOD} 1", "culls 0 garbage 1 keys 1", f"due {NONE} 0", f"due {PERIOD} 1"]
