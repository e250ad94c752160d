"""The binding read from include/stlpose_hip.h (stlpose_amd/capi.py, cheader.py) against what gcc makes of the same header: every
struct's size, every field's offset and size, every constant's value; the argument types of the awkward prototypes spelled out by
hand; and the reader's refusal of anything outside the C subset it knows."""
import ctypes as C
import os
import re
import subprocess

import pytest

from stlpose_amd import capi
from stlpose_amd.cheader import Header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_PATH = os.path.join(ROOT, "include", "stlpose_hip.h")
# C struct -> the name other modules use for its class, written out here so that the pairing itself is checked
CLASSES = {"stl_src": "Src", "stl_conv": "Conv", "stl_wgrad": "Wgrad", "stl_wgrad_io": "WgradIO", "stl_wgrad_group": "WgradGroup",
           "stl_term": "Term", "stl_fuse": "Fuse", "stl_fuse_bwd": "FuseBwd", "stl_upbwd": "UpBwd", "stl_wprep": "WPrep",
           "stl_slab": "Slab", "stl_bnrec": "BNRec", "stl_reduce_range": "ReduceRange", "stl_bn_range": "BNRange",
           "stl_patch": "Patch", "stl_patch_bwd": "PatchBwd", "stl_head": "Head", "stl_head_bwd": "HeadBwd", "stl_op": "Op",
           "StlDetImage": "DetImage", "StlDetPointwise": "DetPointwise", "StlDetTerm": "DetTerm", "StlDetFuse": "DetFuse",
           "StlDetPointwise16": "DetPointwise16", "StlDetPointwiseBwd": "DetPointwiseBwd",
           "StlDetPointwise16Bwd": "DetPointwise16Bwd"}


def _header_text():
    with open(HEADER_PATH) as f:
        return re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)


@pytest.fixture(scope="module")
def gcc_says(tmp_path_factory):
    """{("sizeof", struct): n, ("field", struct, name): (offset, size), ("define", STL_NAME): value} printed by a C program that
    is written from the tables the reader made and compiled against the header itself."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "stlpose_hip.h"', 'int main(void) {']
    for cname, cls in capi.HEADER.structs.items():
        lines.append(f'printf("sizeof {cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("field {cname} {f} %zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname}*)0)->{f}));' for f, _ in cls._fields_]
    lines += [f'printf("define {name} %lld\\n", (long long)({name}));' for name in capi.HEADER.constants]
    d = tmp_path_factory.mktemp("capi_header")
    (d / "layout.c").write_text("\n".join(lines + ["return 0; }"]))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(d / "layout.c"), "-o", str(d / "layout")])
    out = {}
    for kind, *words in map(str.split, subprocess.check_output([str(d / "layout")]).decode().splitlines()):
        if kind == "field":
            out[(kind, words[0], words[1])] = (int(words[2]), int(words[3]))
        else:
            out[(kind, words[0])] = int(words[1])
    return out


def test_every_struct_of_the_header_has_its_class():
    """The typedefs found by a regex of this test's own, their members counted by it, against the classes capi exposes."""
    bodies = {name: body for body, name in re.findall(r"\{([^{}]*)\}\s*(\w+)\s*;", _header_text())}
    assert set(bodies) == set(CLASSES) == set(capi.HEADER.structs) and len(bodies) == 26
    for cname, body in bodies.items():
        cls = getattr(capi, CLASSES[cname])
        assert cls is capi.HEADER.structs[cname] and issubclass(cls, C.Structure) and cls.__name__ == CLASSES[cname]
        members = [d.split()[-1].lstrip("*").split("[")[0] for line in body.split(";") if line.strip() for d in line.split(",")]
        assert [f for f, _ in cls._fields_] == members, cname


def test_struct_layouts_match_gcc(gcc_says):
    """sizeof of every struct, offsetof and sizeof of every field: the ctypes classes have the C layout."""
    for cname, pyname in CLASSES.items():
        cls = getattr(capi, pyname)
        assert C.sizeof(cls) == gcc_says[("sizeof", cname)], cname
        for f, _ in cls._fields_:
            assert (getattr(cls, f).offset, getattr(cls, f).size) == gcc_says[("field", cname, f)], (cname, f)
    assert sum(k[0] == "field" for k in gcc_says) == sum(len(getattr(capi, p)._fields_) for p in CLASSES.values())


def test_constants_match_gcc(gcc_says):
    """Every object-like #define STL_* (found by this test's own regex) has, under its name without STL_, the value gcc gives it."""
    defines = set(re.findall(r"^[ \t]*#define[ \t]+(STL_\w+)[ \t]+\S", _header_text(), flags=re.M))
    assert defines == set(capi.HEADER.constants) and len(defines) == 61 and "STL_DT2" not in defines
    for name in defines:
        assert getattr(capi, name[len("STL_"):]) == capi.HEADER.constants[name] == gcc_says[("define", name)], name
    assert capi.POSE_RANK_ANY_MAX == 1 << 24 and capi.NSHARD == 2 and capi.WGRAD_GROUP_MAX == 8
    assert (capi.F32, capi.BF16, capi.F16, capi.MIXED) == (0, 1, 2, capi.dt2(1, 2)) == (0, 1, 2, 0x201)
    # the caps of the pose scoring, which keypoint_eval.py sizes its tables by
    assert (capi.POSE_JOINTS, capi.POSE_NMS_MAX, capi.OKS_AP_THRS, capi.OKS_AP_AREAS, capi.OKS_AP_DETS) == tuple(
        gcc_says[("define", n)] for n in ("STL_POSE_JOINTS", "STL_POSE_NMS_MAX", "STL_OKS_AP_THRS", "STL_OKS_AP_AREAS", "STL_OKS_AP_DETS"))


def test_op_kinds_and_string_maps_take_their_numbers_from_the_header(gcc_says):
    """OP_KIND covers exactly the STL_OP_* values; a new op kind is appended, not renumbered (11 and 12 stay retired)."""
    kinds = {v for k, v in gcc_says.items() if k[0] == "define" and k[1].startswith("STL_OP_")}
    assert kinds == set(capi.OP_KIND.values()) == set(range(11)) | {13} and len(capi.OP_KIND) == 12
    assert gcc_says[("define", "STL_OP_PATCH_BWD")] == capi.OP_KIND["stl_patch3x3_backward"] == 13
    assert gcc_says[("sizeof", "stl_patch_bwd")] == C.sizeof(capi.PatchBwd)
    assert (capi.OP_KIND["stl_conv_forward"], capi.OP_KIND["stl_conv_wgrad"], capi.OP_KIND["stl_conv_wgrad_group"]) == (0, 1, 10)
    assert capi.POSE_APPROACH == {"all_kpts": 0, "full_body": 1, "upper_body": 2}
    assert capi.POSE_METHOD == {"euclidean": 0, "cosine": 1, "manhattan": 2, "confidence": 3, "oks": 4, "l2sq": 5, "cos_normalised": 6}
    assert capi.POSE_PEN == {"zero_coord": 0, "none": 1, "mean": 2, "max": 3} and capi.POSE_SUM_ORDER == {"numpy": 0, "reference": 1}


def test_awkward_prototypes_are_read_as_written_here():
    vp, i32, i64, f32, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double
    expected = {
        "stl_pose_augment": ([vp, vp, vp, vp, vp, i64, vp, vp, i32, i32, i32, f64, f64, i32, f64, i32, i32,
                              vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp], C.c_int),
        "stl_bn_running_update": ([vp, vp, vp, vp, i32, f32, vp, vp], C.c_int),     # comments inside the list
        "stl_program_run": ([vp, vp], C.c_int),                                     # void* const*
        "stl_box_select": ([vp, vp, vp, vp, i32, i64, i32, i64, i32, f32, f64, vp, vp, vp], C.c_int),
        "stl_conv_wgrad_group": ([C.POINTER(capi.WgradGroup), vp], C.c_int),        # a host descriptor
        "stl_weight_prep": ([i32, vp, vp, vp, i32, i32, vp], C.c_int),              # const stl_wprep*: a device table
        "stl_det_nms_workspace": ([i32], C.c_int64),
        "stl_last_error": ([], C.c_char_p),
    }
    for name, (argtypes, restype) in expected.items():
        assert capi.SIGNATURES[name] == argtypes and capi.RESTYPES[name] is restype, name
    assert len(capi.SIGNATURES["stl_pose_augment"]) == 28
    assert capi.SIGNATURES["stl_program_create"][0] is C.POINTER(capi.Op)
    assert dict(capi.WgradGroup._fields_)["p"] is C.POINTER(capi.Wgrad) * 8 and dict(capi.ReduceRange._fields_)["tab"] is vp
    assert set(capi.INT64_FUNCS) == {"stl_det_nms_workspace", "stl_pose_rank_any_workspace"}
    assert set(capi.STRING_FUNCS) == {"stl_last_error", "stl_build_id", "stl_last_kernel"}
    assert len(capi.SIGNATURES) == 98 and set(capi.RESTYPES) == set(capi.SIGNATURES)
    assert capi.DEBUG_SIGNATURES == {n: [vp] for n in ("stl_debug_conv_stamps", "stl_debug_conv_stamps2", "stl_debug_wgrad_stamps",
                                                       "stl_debug_wgrad_stamps2")}


@pytest.mark.parametrize("line, why", [
    ("static int stl_hidden;", "outside the C subset"),
    ("#pragma once", "outside the C subset"),
    ("#define STL_WIDE sizeof(int)", "not an integer expression"),
    ("int stl_f(size_t n);", "unknown type 'size_t'"),
    ("void stl_f(int n);", "outside the C subset"),
    ("int stl_f(int);", "cannot read the declaration 'int'"),
    ("typedef struct { float *a, b; } stl_two;", "cannot read the declaration"),
    ("typedef struct { int32_t v[STL_MISSING]; } stl_arr;", "unknown array extent 'STL_MISSING'"),
    ("typedef struct { stl_later s; } stl_nest;", "unknown type 'stl_later'"),
])
def test_reader_refuses_what_it_does_not_know(tmp_path, line, why):
    """A header edit outside the subset fails at import with the line, it does not drop a symbol."""
    good = "/* c */\n#define STL_N 3 /* n\n more */\ntypedef struct stl_a { int32_t x, y[STL_N]; const void* p; } stl_a;\n"
    (tmp_path / "h.h").write_text(good + line + "\nint stl_g(const stl_a* a, void* const* s /* or NULL */);\n")
    with pytest.raises(SyntaxError, match=re.escape(why)) as e:
        Header(str(tmp_path / "h.h"))
    assert f"h.h:5: " in str(e.value) and repr(line) in str(e.value)
    (tmp_path / "h.h").write_text(good + "int stl_g(const stl_a* a, void* const* s /* or NULL */);\n")
    h = Header(str(tmp_path / "h.h"))
    assert h.constants == {"STL_N": 3} and h.signatures == {"stl_g": [C.POINTER(h.structs["stl_a"]), C.c_void_p]}
    assert [(f, C.sizeof(t)) for f, t in h.structs["stl_a"]._fields_] == [("x", 4), ("y", 12), ("p", 8)]
