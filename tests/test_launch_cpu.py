"""CPU: ``stlpose_amd.launch.LaunchList`` -- how ``add`` converts and keeps its arguments, the error path of ``run`` (descriptors
that fail the library's first host-side check: nothing is launched), slicing and selection -- and the launch plans of the
Python-listed models against the signatures recorded before they moved onto it (tests/golden/launch/plans.json), and the detector's training lists at every depth, with the
buffer behind each pointer, against those recorded before one builder per stage listed them (detector_train.json)."""
import ctypes as C
import json
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def built_lib():
    from stlpose_amd import build
    build.build(verbose=False)
    from stlpose_amd import capi
    return capi.lib()


def _bad_conv(**fields):
    """A conv descriptor that fails stl_conv_forward's host-side checks."""
    from stlpose_amd import capi
    p = capi.Conv()
    p.dtype, p.B, p.Hi, p.Wi, p.Ci, p.Ho, p.Wo, p.Co, p.ks, p.stride, p.shape = capi.F32, 1, 8, 8, 32, 8, 8, 32, 3, 1, -1
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def test_add_converts_and_keeps(built_lib):
    from stlpose_amd import capi
    from stlpose_amd.launch import LaunchList
    t, p, vp = torch.zeros(4), capi.Conv(), C.c_void_p(24)
    ll = LaunchList()
    ll.add("stl_conv_forward", t, p, None, 7, 0.5, vp, t.data_ptr() + 8)
    (fn, name, args), = ll.calls
    assert name == "stl_conv_forward" and fn is built_lib.stl_conv_forward
    assert isinstance(args[0], C.c_void_p) and args[0].value == t.data_ptr() and any(k is t for k in ll.keep)
    assert args[1]._obj is p and any(k is p for k in ll.keep)          # by reference: the very object, not a copy
    p.Co = 77                                                           # what HeadTrain.set_grads relies on
    assert args[1]._obj.Co == 77 and [k for k in ll.keep if isinstance(k, capi.Conv)][0].Co == 77
    assert args[2] is None and args[3] == 7 and type(args[3]) is int and args[4] == 0.5 and type(args[4]) is float
    assert args[5] is vp and args[6] == t.data_ptr() + 8 and type(args[6]) is int
    assert len(ll.keep) == 2                                            # nothing else is kept
    owner = torch.zeros(2)
    ll.keep_alive(owner, None)
    assert ll.keep[-1] is owner and len(ll.keep) == 3


def test_lists_of_one_plan_share_keep(built_lib):
    from stlpose_amd.launch import LaunchList
    a = LaunchList()
    b = LaunchList(a.keep)
    assert b.keep is a.keep and LaunchList().keep is not a.keep
    t = torch.zeros(1)
    b.add("stl_maxpool2x2", 0, t, t, 1, 2, 2, 8)
    assert a.keep[0] is t and len(a) == 0 and len(b) == 1


def test_run_raises_the_first_error_and_stops(built_lib):
    from stlpose_amd.launch import LaunchList
    ll = LaunchList()
    ll.add("stl_conv_forward", _bad_conv(dtype=99))
    ll.add("stl_conv_forward", _bad_conv(ks=5))
    with pytest.raises(RuntimeError) as ei:
        ll.run(0)
    msg = str(ei.value)
    assert "stl_conv_forward" in msg and "bad dtype" in msg and "ks must be 1 or 3" not in msg
    assert "bad dtype" in built_lib.stl_last_error().decode()          # the second entry was never called
    with pytest.raises(RuntimeError, match="ks must be 1 or 3"):       # ... and is reached when the slice starts at it
        ll.run(0, 1)


def test_slices_selection_len_and_names(built_lib):
    from stlpose_amd.launch import LaunchList
    ll = LaunchList()
    ll.add("stl_conv_forward", _bad_conv(dtype=99))
    ll.add("stl_maxpool2x2", 99, 0, 0, 1, 2, 2, 8)
    ll.add("stl_conv_forward", _bad_conv(ks=5))
    for i in range(4):
        ll.run(0, i, i)                                                 # an empty slice calls nothing: no error
    ll.run(0, 3)
    assert len(ll) == 3 == len(ll.names()) and ll.names() == ["stl_conv_forward", "stl_maxpool2x2", "stl_conv_forward"]
    assert [(name, args) for _, name, args in ll] == [(c[1], c[2]) for c in ll.calls]
    sel = ll.select(lambda n: n == "stl_conv_forward")
    assert sel.keep is ll.keep and sel.calls == [ll.calls[0], ll.calls[2]] and len(ll) == 3
    assert ll.select(lambda n: False).names() == []
    with pytest.raises(RuntimeError, match="ks must be 1 or 3"):
        sel.run(0, 1, 2)


@pytest.mark.parametrize("model", ["vgg16", "vgg19", "adain", "d0.fp32", "d0.bf16", "d0.f16"])
def test_plans_are_the_recorded_ones(model, built_lib):
    """Every list holds the same ordered entry points with the same arguments (tests/launch_plans.py: scalars, descriptor fields,
    which pointers are null) as on the commit plans.json was recorded from, and the detector's counters are the same."""
    from tests import launch_plans
    want = json.load(open(os.path.join(HERE, "golden", "launch", "plans.json")))["plans"]
    got = launch_plans.BUILDERS[model]()
    assert set(got) == {k for k in want if k.startswith(model) or (model == "d0.fp32" and k.startswith("d0.train"))}
    for key, g in got.items():
        w = want[key]
        if isinstance(w, dict):
            assert g["names"] == w["names"], key
            diff = [i for i, (a, b) in enumerate(zip(g["crc"], w["crc"])) if a != b]
            assert not diff, f"{key}: arguments of entry {diff[0]} ({g['names'][diff[0]]}) changed"
        else:
            assert g == w, key


def _detector_train_keys():
    from tests import launch_plans
    return list(launch_plans.DETECTOR_TRAIN)


@pytest.mark.parametrize("key", _detector_train_keys())
def test_detector_training_lists_are_the_recorded_ones(key, built_lib):
    """The detector's training forward and backward at every depth (tests/launch_plans.py: DETECTOR_TRAIN) hold the same ordered
    entry points with the same arguments as on the commit detector_train.json was recorded from, every pointer names the same
    buffer with the same room behind it, and no pointer lies outside the tensors that the plan keeps (launch_plans.aliasing)."""
    from tests import launch_plans
    want = json.load(open(os.path.join(HERE, "golden", "launch", "detector_train.json")))["plans"][key]
    got = launch_plans.detector_train(key)
    assert set(got) == set(want) == {"fwd", "bwd"}
    for which in ("fwd", "bwd"):
        g, w = got[which], want[which]
        for i, (gn, wn) in enumerate(zip(g["names"], w["names"])):
            assert gn == wn, f"{key}: {which}[{i}] is {gn}, recorded {wn}"
        assert len(g["names"]) == len(w["names"]), f"{key}: {which} has {len(g['names'])} entries, recorded {len(w['names'])}"
        for i, name in enumerate(g["names"]):
            assert g["crc"][i] == w["crc"][i], f"{key}: {which}[{i}] ({name}): its arguments changed"
            assert g["alias"][i] == w["alias"][i], f"{key}: {which}[{i}] ({name}): a pointer names another buffer, or the room behind one changed"
