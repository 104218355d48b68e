"""What the map-set analysis calls do alike around their kernels ("The frame of a map-set call"): a context's scratch
made whole by a first call that fails, the tally cleared per call, when the stats become valid, the output's own path, the live model
in or out of the set.  sm_set_call.h has ten users; seven are run here (sm_simplify_maps, sm_register_maps, sm_compare_maps,
sm_tile_maps, sm_segment_maps, sm_mesh_maps, sm_ground_maps), each on a context of its own; sm_locate_maps, sm_cast_rays_maps and
sm_query_points_maps stand with them in tests/test_call_order.py, which runs every call after every other.  What the calls compute is
their own tests' business; here one call is held against another call of the same library, so the file passes unchanged on the
library before the frame and on the one after it (SM_HIP_LIB selects a build).  _run and _counts live in tests/call_probes.py."""
import os

import numpy as np
import pytest

import recall_ref as cr
import test_simplify as ts
from call_probes import counts as _counts, run_analysis as _run

pytestmark = pytest.mark.gpu

# three files -- one of a single partial block of 256 records, one of a block and a part, one of several -- and a live model
FILE_ROWS = (200, 300, 400)
LIVE_ROWS = 200
CALLS = ("simplify", "register", "compare", "tile", "segment", "mesh", "ground")
# a first call's refusal: the one capacity a call has at 1 (SM_E_CAPACITY, known once the set has been read); the ground map has
# none, a parameter out of range stands in (SM_E_ARG, before the set is opened)
BAD = dict(simplify=dict(max_cells=1), register=dict(max_cells=1), compare=dict(max_cells=1), tile=dict(max_tiles=1), segment=dict(max_cells=1),
           mesh=dict(max_cells=1), ground=dict(cell_mm=9))
# sm_*_stats after that refusal: five calls reset their stats and set them valid once the set is open, two publish them on success
STATS_AFTER_REFUSAL = dict(simplify=True, register=True, compare=True, tile=True, segment=True, mesh=False, ground=False)
# the calls that write to a path the caller names
WRITES = ("simplify", "compare", "tile", "segment", "mesh")


@pytest.fixture(scope="module")
def rows():
    r = ts.Scene().rows
    assert len(r) >= sum(FILE_ROWS) + LIVE_ROWS
    return r[:sum(FILE_ROWS) + LIVE_ROWS]


class Sets:
    """the set of three files, and a second set of the same records moved by 3 cm for the calls on two sets"""

    def __init__(self, folder, rows):
        self.folder = str(folder)
        cuts = np.cumsum(FILE_ROWS)
        parts = np.split(rows, cuts)
        self.live = parts[3]
        self.paths = [os.path.join(self.folder, "tile_%06d.bin" % i) for i in range(3)]     # (names a tiling with the prefix "tile" gives)
        for i, p in enumerate(self.paths):
            cr.write_map(p, parts[i], 10 + i, 20 + i)
        moved = rows[:cuts[2]].copy()
        moved[:, 0] += np.float32(0.03)
        self.other = [os.path.join(self.folder, "other%d.bin" % i) for i in range(2)]
        for p, part in zip(self.other, np.split(moved, [450])):
            cr.write_map(p, part, 30, 40)
        self.file_records = int(cuts[2])
        self.n_out = 0

    def out(self):
        self.n_out += 1
        return os.path.join(self.folder, "out%d" % self.n_out)

    def bytes(self):
        return [open(p, "rb").read() for p in self.paths + self.other]

    def no_tmp(self):
        ts._no_tmp(self.folder)


def _stats(m, call):
    return getattr(m, call + "_stats")()


def _refused(m, call, sets, **kw):
    from surfelmapping_amd import capi
    with pytest.raises(capi.SurfelMapError) as e:
        _run(m, call, sets, **kw)
    return e.value


@pytest.mark.parametrize("call", CALLS)
def test_good_call_after_a_refused_first_call(call, rows, tmp_path):
    """the scratch is whole and the tally clear whatever the context's first call came to; no temporary is left"""
    from surfelmapping_amd import capi
    sets = Sets(tmp_path, rows)
    fresh, used = ts._ctx(sets.live), ts._ctx(sets.live)
    want, _ = _run(fresh, call, sets)
    before = sorted(os.listdir(tmp_path))
    e = _refused(used, call, sets, **BAD[call])
    assert e.rc == (capi.SM_E_ARG if call == "ground" else capi.SM_E_CAPACITY), e
    assert sorted(os.listdir(tmp_path)) == before                             # (nothing written, nothing left)
    got, _ = _run(used, call, sets)
    assert got == want
    assert _counts(_stats(used, call)) == _counts(_stats(fresh, call))
    sets.no_tmp()
    fresh.close()
    used.close()


@pytest.mark.parametrize("call", CALLS)
def test_same_call_twice(call, rows, tmp_path):
    sets = Sets(tmp_path, rows)
    m = ts._ctx(sets.live)
    first, _ = _run(m, call, sets)
    st = _counts(_stats(m, call))
    second, _ = _run(m, call, sets)
    assert second == first and _counts(_stats(m, call)) == st
    sets.no_tmp()
    m.close()


@pytest.mark.parametrize("call", CALLS)
def test_when_stats_are_valid(call, rows, tmp_path):
    """before any call, after a first call that is refused, after one that succeeds"""
    from surfelmapping_amd import capi
    sets = Sets(tmp_path, rows)
    m = ts._ctx(sets.live)
    with pytest.raises(capi.SurfelMapError) as e:
        _stats(m, call)
    assert e.value.rc == capi.SM_E_ARG and "call yet" in str(e.value)
    _refused(m, call, sets, **BAD[call])
    if STATS_AFTER_REFUSAL[call]:
        st = _stats(m, call)                                                  # what the call had tallied when it was refused
        total = sets.file_records + LIVE_ROWS
        seen = st["source_records"] if call == "register" else st["records_in"] if call in ("simplify", "tile") else None
        assert seen in (None, total) and st["total_ms"] == 0.0
    else:
        with pytest.raises(capi.SurfelMapError) as e:
            _stats(m, call)
        assert e.value.rc == capi.SM_E_ARG and "call yet" in str(e.value)
    _run(m, call, sets)
    st = _stats(m, call)
    assert st["total_ms"] > 0.0 and st["chunks"] > 0 and st["launches"] > 0
    m.close()


@pytest.mark.parametrize("call", WRITES)
def test_output_needs_a_path_of_its_own(call, rows, tmp_path):
    from surfelmapping_amd import capi
    sets = Sets(tmp_path, rows)
    m = ts._ctx(sets.live)
    before, listing = sets.bytes(), sorted(os.listdir(tmp_path))
    # (a tiling names its files itself: with this prefix the first is the set's first file)
    taken = os.path.join(sets.folder, "tile") if call == "tile" else sets.paths[1]
    e = _refused(m, call, sets, out=taken)
    assert e.rc == capi.SM_E_ARG and "of its own" in str(e)
    assert sets.bytes() == before and sorted(os.listdir(tmp_path)) == listing
    m.close()


@pytest.mark.parametrize("call", CALLS)
def test_live_model_in_and_out_of_the_set(call, rows, tmp_path):
    sets = Sets(tmp_path, rows)
    m = ts._ctx(sets.live)
    assert m.counts()["count"] == LIVE_ROWS
    assert _run(m, call, sets, include_model=True)[1] == sets.file_records + LIVE_ROWS
    assert _run(m, call, sets, include_model=False)[1] == sets.file_records
    assert _run(m, call, sets, include_model=True)[1] == sets.file_records + LIVE_ROWS
    m.close()
