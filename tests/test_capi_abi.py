"""The whole C-ABI boundary of surfelmapping_amd/capi.py against the C compiler's view of include/sm_c_api.h, without a GPU: the
layout of EVERY ctypes structure the module defines (found in the module, so a new one is covered unasked), the numpy record types,
the header's constants that capi mirrors, and the prototype table -- names, parameter counts and return kinds -- against the
header's declarations.  One generated C program, one compile."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

import ground_ref as gr
import place_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def _constants(capi):
    """the header's constants that capi holds a copy of: C expression -> the copy"""
    return {
        "SM_API_VERSION": capi.API_VERSION,
        "SM_OK": capi.SM_OK, "SM_E_ARG": capi.SM_E_ARG, "SM_E_CAPACITY": capi.SM_E_CAPACITY, "SM_E_UNSUPPORTED": capi.SM_E_UNSUPPORTED,
        "SM_E_HIP": capi.SM_E_HIP, "SM_E_NO_DEVICE": capi.SM_E_NO_DEVICE,
        "SM_FRAME_LOG_LEN": capi.FRAME_LOG_LEN,
        "SM_TRACK_OK": capi.SM_TRACK_OK, "SM_TRACK_LOST": capi.SM_TRACK_LOST, "SM_TRACK_DEGENERATE": capi.SM_TRACK_DEGENERATE,
        "SM_TRACK_NO_MODEL": capi.SM_TRACK_NO_MODEL,
        "SM_RECALL_MOVE": capi.SM_RECALL_MOVE, "SM_RECALL_COPY": capi.SM_RECALL_COPY, "SM_RECALL_COUNT": capi.SM_RECALL_COUNT,
        "SM_LOOP_CLOSED": capi.SM_LOOP_CLOSED, "SM_LOOP_NONE": capi.SM_LOOP_NONE, "SM_LOOP_NO_OLD_MAP": capi.SM_LOOP_NO_OLD_MAP,
        "SM_LOOP_TRACK_FAILED": capi.SM_LOOP_TRACK_FAILED, "SM_LOOP_REJECTED": capi.SM_LOOP_REJECTED,
        "SM_SEARCH_MAX_CANDIDATES": capi.SEARCH_MAX_CANDIDATES, "SM_LIDAR_MAX_BEAMS": capi.LIDAR_MAX_BEAMS,
        "SM_FERN_MAX_KEYFRAMES": capi.FERN_MAX_KEYFRAMES, "SM_RAYS_MAX": capi.RAYS_MAX,
        "SM_SCENE_MAX_ACTORS": capi.SCENE_MAX_ACTORS, "SM_SCENE_MAX_RECORDS": capi.SCENE_MAX_RECORDS,
        "SM_REGISTER_OK": capi.SM_REGISTER_OK, "SM_REGISTER_LOST": capi.SM_REGISTER_LOST, "SM_REGISTER_DEGENERATE": capi.SM_REGISTER_DEGENERATE,
        "SM_REGISTER_NO_TARGET": capi.SM_REGISTER_NO_TARGET, "SM_REGISTER_NO_SOURCE": capi.SM_REGISTER_NO_SOURCE,
        "SM_REGISTER_MAX_LEVELS": capi.REGISTER_MAX_LEVELS,
        "SM_COMPARE_SUPPORTED": capi.SM_COMPARE_SUPPORTED, "SM_COMPARE_CHANGED": capi.SM_COMPARE_CHANGED,
        "SM_COMPARE_OUTSIDE": capi.SM_COMPARE_OUTSIDE, "SM_COMPARE_LOOSE": capi.SM_COMPARE_LOOSE,
        "SM_SEGMENT_LOOSE": capi.SM_SEGMENT_LOOSE, "SM_SEGMENT_SMALL": capi.SM_SEGMENT_SMALL, "SM_SEGMENT_SKIPPED": capi.SM_SEGMENT_SKIPPED,
        "SM_GROUND_NONE": capi.GROUND_NONE,
    }


# ... and the values the per-feature tests held them against, written out
LITERALS = {
    "SM_API_VERSION": 4,
    "SM_TRACK_OK": 0, "SM_TRACK_LOST": 1, "SM_TRACK_DEGENERATE": 2, "SM_TRACK_NO_MODEL": 3,
    "SM_RECALL_MOVE": 0, "SM_RECALL_COPY": 1, "SM_RECALL_COUNT": 2,
    "SM_LOOP_CLOSED": 0, "SM_LOOP_NONE": 1, "SM_LOOP_NO_OLD_MAP": 2, "SM_LOOP_TRACK_FAILED": 3, "SM_LOOP_REJECTED": 4,
    "SM_REGISTER_OK": 0, "SM_REGISTER_LOST": 1, "SM_REGISTER_DEGENERATE": 2, "SM_REGISTER_NO_TARGET": 3, "SM_REGISTER_NO_SOURCE": 4,
    "SM_COMPARE_SUPPORTED": 0, "SM_COMPARE_CHANGED": 1, "SM_COMPARE_OUTSIDE": 2, "SM_COMPARE_LOOSE": 3,
    "SM_SCENE_MAX_ACTORS": 4096, "SM_SCENE_MAX_RECORDS": 4194304, "SM_RAYS_MAX": 1 << 24,
    "SM_GROUND_NONE": gr.NONE,
}
# the structures whose size other code relies on (a record stride, a file layout)
SIZES = {"sm_segment_component": 64, "sm_mesh_vertex": 28, "sm_ray": 32, "sm_stereo_params": 28, "sm_fern": 12}


def header_code():
    """the header without its comments"""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "sm_c_api.h")).read(), flags=re.S)


def header_typedefs():
    return set(re.findall(r"typedef\s+struct\s+(sm_\w+)\s*\{", header_code()))


def header_declarations():
    """{function: (return type, number of parameters)} of every function the header declares"""
    out = {}
    for ret, name, params in re.findall(r"^[ \t]*((?:const\s+)?\w+(?:\s+\w+)*[\s*]+)(sm_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header_code(), flags=re.M):
        if ret.split()[0] == "typedef":
            continue
        params = params.strip()
        out[name] = (" ".join(ret.split()), 0 if params in ("", "void") else len(params.split(",")))
    return out


def structures():
    """every ctypes.Structure subclass capi defines, by name"""
    from surfelmapping_amd import capi
    return dict(inspect.getmembers(capi, lambda o: inspect.isclass(o) and issubclass(o, C.Structure) and o.__module__ == capi.__name__))


def typedef_of(name, typedefs):
    """SmFooBar -> sm_foo_bar or sm_foo_bar_t, whichever the header has; neither or both is an error"""
    assert name.startswith("Sm"), name
    snake = "sm" + re.sub(r"([A-Z])", lambda m: "_" + m.group(1).lower(), name[2:])
    found = [t for t in (snake, snake + "_t") if t in typedefs]
    assert len(found) == 1, f"{name}: {len(found)} typedefs of include/sm_c_api.h match ({snake}, {snake}_t): {found}"
    return found[0]


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """what gcc says: {"sm_x": sizeof, "sm_x.field": offsetof, "SM_CONSTANT": value}, from one program"""
    from surfelmapping_amd import capi
    typedefs = header_typedefs()
    lines = []
    for name, cls in structures().items():
        cname = typedef_of(name, typedefs)
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{n} %zu\\n", offsetof({cname}, {n}));' for n, *_ in cls._fields_]
    lines.append('printf("sm_frame_log %zu\\n", sizeof(sm_frame_log));')
    lines += [f'printf("{c} %lld\\n", (long long)({c}));' for c in _constants(capi)]
    tmp = tmp_path_factory.mktemp("abi")
    src = tmp / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sm_c_api.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    subprocess.check_call(["gcc", "-I", INCLUDE, "-o", str(tmp / "layout"), str(src)])
    return {k: int(v) for k, v in (l.split() for l in subprocess.check_output([str(tmp / "layout")]).decode().splitlines())}


def test_every_structure_has_the_header_layout(compiled):
    typedefs = header_typedefs()
    found = structures()
    assert len(found) >= 58
    used = {}
    for name, cls in found.items():
        cname = typedef_of(name, typedefs)
        assert used.setdefault(cname, name) == name, f"{cname} is mirrored twice: {used[cname]}, {name}"
        assert compiled[cname] == C.sizeof(cls), (cname, compiled[cname], C.sizeof(cls))
        for n, *_ in cls._fields_:
            assert compiled[f"{cname}.{n}"] == getattr(cls, n).offset, f"{cname}.{n}"
    for cname, size in SIZES.items():
        assert compiled[cname] == size, cname


def test_numpy_record_types_have_the_header_layout(compiled):
    from surfelmapping_amd import capi
    assert capi.FRAME_LOG_DTYPE.itemsize == compiled["sm_frame_log"]
    for dtype, cls, cname in ((capi.SEGMENT_COMPONENT, capi.SmSegmentComponent, "sm_segment_component"), (capi.MESH_VERTEX, capi.SmMeshVertex, "sm_mesh_vertex"),
                              (capi.FERN_DTYPE, capi.SmFern, "sm_fern")):
        assert dtype.itemsize == C.sizeof(cls) == compiled[cname], cname
        assert list(dtype.names) == [n for n, _ in cls._fields_], cname
        for n in dtype.names:
            assert dtype.fields[n][1] == getattr(cls, n).offset == compiled[f"{cname}.{n}"], (cname, n)
    assert capi.FERN_DTYPE.itemsize == pr.FERN_DTYPE.itemsize == 12


def test_header_constants_match_their_copies(compiled):
    from surfelmapping_amd import capi
    for c, value in _constants(capi).items():
        assert compiled[c] == value, (c, compiled[c], value)
    for c, value in LITERALS.items():
        assert compiled[c] == value, (c, compiled[c], value)
    assert [capi.REGISTER_STATUS[i] for i in range(5)] == ["OK", "LOST", "DEGENERATE", "NO_TARGET", "NO_SOURCE"]
    assert capi.RAYS_MAX == 1 << 24 and capi.GROUND_NONE == gr.NONE


def test_prototype_table_matches_the_header_declarations():
    from surfelmapping_amd import capi
    declared = header_declarations()
    names = sorted(set(re.findall(r"\b(sm_[a-z0-9_]+)\s*\(", header_code())))
    assert sorted(declared) == names                                # the declaration pattern misses no function of the header
    assert sorted(capi.SYMBOLS) == names and len(set(capi.SYMBOLS)) == len(capi.SYMBOLS)
    assert set(capi.PROTOTYPES) == set(capi.SYMBOLS) | set(capi.DIAGNOSTICS) and not set(capi.SYMBOLS) & set(capi.DIAGNOSTICS)
    for name, (ret, n_params) in declared.items():
        restype, argtypes = capi.PROTOTYPES[name]
        assert len(argtypes) == n_params, (name, len(argtypes), n_params)
        if "*" in ret:
            assert restype in (C.c_void_p, C.c_char_p), (name, ret, restype)
        elif ret == "void":
            assert restype is None, (name, restype)
        else:
            assert ret == "int" and restype is C.c_int, (name, ret, restype)


def test_load_gives_every_function_its_row():
    from surfelmapping_amd import capi
    L = capi.load()
    for name, (restype, argtypes) in capi.PROTOTYPES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_diagnostics_are_exported_and_not_in_the_header():
    from surfelmapping_amd import capi
    L = capi.load()
    code = header_code()
    assert len(capi.DIAGNOSTICS) == 7
    for name in capi.DIAGNOSTICS:
        assert name.startswith("sm_debug_") and hasattr(L, name), name
        assert name not in capi.SYMBOLS and not re.search(r"\b" + name + r"\b", code), name
