"""CPU: the host halves of the detector's device tail (stlpose_amd/detections.py), the argument checks of its public switches, the
dispatcher's refusal of CPU tensors and the reading of include/stlpose_hip_detections.h."""
import ctypes as C

import numpy as np
import pytest
import torch

import stlpose_amd  # noqa: F401  (registers the stlpose:: ops)
from stlpose_amd import DetectorEvaluator, capi, efficientdet as E, ops
from stlpose_amd.detections import Detections, DetectionStore

K = capi.BOX_MAX


def _tables(counts):
    """Hand-filled CPU tables: row r of image i is box (i, r, i + r + 1, 2r + 2), score 1 - r / 8192, label 1 + (r + i) % 3."""
    b = len(counts)
    r = torch.arange(K, dtype=torch.float32)
    boxes = torch.stack([torch.stack([torch.full((K,), float(i)), r, i + r + 1, 2 * r + 2], 1) for i in range(b)])
    scores = (1 - r / 8192).repeat(b, 1)
    labels = torch.stack([1 + (torch.arange(K, dtype=torch.int32) + i) % 3 for i in range(b)]).to(torch.int32)
    return Detections(boxes, scores, labels, torch.tensor(counts, dtype=torch.int32))


def test_output_switches_refuse_other_values():
    m = E.setup_detector("efficientdet", "d0").eval()
    with pytest.raises(ValueError, match="output 'x'"):
        m(torch.zeros(1, 3, 64, 64), output="x")
    with pytest.raises(ValueError, match="output 'x'"):
        m.detect(None, None, 0.5, 0.5, output="x")
    with pytest.raises(ValueError, match="output 'x'"):
        DetectorEvaluator(m, device="cpu", output="x")
    from stlpose_amd.topdown import detect_poses
    with pytest.raises(ValueError, match="pipeline 'x'"):
        detect_poses(m, None, [], pipeline="x")
    assert DetectorEvaluator(m, device="cpu").output == "host" and DetectorEvaluator(m, device="cpu", output="device").output == "device"


def test_to_list_from_host_tables():
    out = _tables([3, 0, K]).to_list()
    assert [len(d["scores"]) for d in out] == [3, 0, K]
    d = out[0]
    assert d["boxes"].dtype == torch.float32 and d["labels"].dtype == torch.int32 and d["scores"].dtype == torch.float32
    assert d["boxes"].tolist() == [[0., 0., 1., 2.], [0., 1., 2., 4.], [0., 2., 3., 6.]] and d["labels"].tolist() == [1, 2, 3]
    assert d["scores"].tolist() == [1.0, 1 - 1 / 8192, 1 - 2 / 8192]
    e = out[1]   # the empty image, as forward writes it: three empty 1-D tensors
    assert e["boxes"].shape == (0,) and e["labels"].shape == (0,) and e["scores"].shape == (0,)
    assert e["boxes"].dtype == torch.float32 and e["labels"].dtype == torch.int32
    assert out[2]["boxes"].shape == (K, 4) and out[2]["labels"][1] == 1
    with pytest.raises(ValueError, match=rf"image 1 of the batch has 5000 candidates .* at most {K} \(STL_BOX_MAX\)"):
        _tables([3, -5001, 2]).to_list()
    with pytest.raises(ValueError, match="Detections: boxes"):
        Detections(torch.zeros(2, K, 4), torch.zeros(2, K), torch.zeros(3, K, dtype=torch.int32), torch.zeros(2, dtype=torch.int32))


def _slot_table(slots, cursor, appends, overflow=0):
    t = np.zeros((1 + len(slots), 3), np.int64)
    t[0, appends & 1], t[0, 2] = cursor, overflow
    t[1:] = np.asarray(slots, np.int64).reshape(-1, 3)
    return t


def test_store_finish_from_a_host_slot_table():
    store = DetectionStore(16, "cpu")
    assert store.boxes.dtype == torch.float64 and store.scores.dtype == torch.float32 and store.labels.dtype == torch.int64
    store.boxes[:] = torch.arange(64, dtype=torch.float64).reshape(16, 4)
    ids, cnt, boxes, scores, labels = store.tables_of(_slot_table([(7, 0, 3), (2, 3, 0), (9, 3, 4)], 7, 3), 3)
    assert ids.tolist() == [7, 2, 9] and cnt.tolist() == [3, 0, 4] and ids.dtype == cnt.dtype == np.int64
    assert boxes.shape == (7, 4) and scores.shape == (7,) and labels.shape == (7,) and boxes[6, 3] == 27
    ids, cnt, boxes, _, _ = store.tables_of(_slot_table([], 0, 0), 0)
    assert len(ids) == 0 and boxes.shape == (0, 4)
    with pytest.raises(ValueError, match=r"capacity of 16 rows was exceeded \(20 rows appended\)"):
        store.tables_of(_slot_table([(7, 0, 12), (2, 12, 8)], 20, 1, overflow=1), 1)
    with pytest.raises(ValueError, match=rf"image id 2 has 4097 candidates .* at most {K} \(STL_BOX_MAX\)"):
        store.tables_of(_slot_table([(7, 0, 3), (2, 3, -4098)], 3, 1), 1)
    with pytest.raises(ValueError, match="image ids for a batch"):
        store.append([1, 2], _tables([1, 1, 1]))
    with pytest.raises(ValueError, match="capacity_rows"):
        DetectionStore(-1, "cpu")


def test_new_ops_have_no_cpu_kernel():
    assert "det_postprocess" in ops.OPS and "det_append" in ops.OPS and "person_boxes" in ops.OPS
    t = _tables([2])
    with pytest.raises(NotImplementedError, match="CPU"):
        torch.ops.stlpose.person_boxes(t.boxes, t.scores, t.labels, t.count, 1, 0.7, -1.0, 0.75, 192, 256)
    with pytest.raises(NotImplementedError, match="CPU"):
        torch.ops.stlpose.det_postprocess(torch.zeros(1, 8, 4), torch.zeros(1, 8, 2), torch.zeros(8, 4), None, 0.5, 511.0, 511.0, 0.5)
    d = _tables([1])
    store = DetectionStore(4, "cpu")
    with pytest.raises(NotImplementedError, match="CPU"):
        store.append([3], d)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        b, s, l, c = torch.ops.stlpose.det_postprocess(torch.empty(2, 8, 4, device="cuda"), torch.empty(2, 8, 3, device="cuda"),
                                                       torch.empty(8, 4, device="cuda"), None, 0.5, 511.0, 511.0, 0.5)
        assert b.shape == (2, K, 4) and s.shape == (2, K) and l.dtype == torch.int32 and c.shape == (2,)


def test_detections_header_is_read():
    vp, i32, i64, f32, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double
    h = capi.DETECTIONS
    assert h.signatures == {
        "stl_det_postprocess": [vp, vp, vp, vp, i32, i32, i32, f32, f32, f32, f64, vp, vp, vp, vp, vp],
        "stl_det_append": [vp, vp, vp, vp, vp, i32, vp, vp, vp, i64, vp, i64, vp, i32, vp, vp],
        "stl_person_boxes": [vp, vp, vp, vp, i32, i32, f32, f64, f32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "stl_person_boxes_workspace": [i32, i32]}
    assert {n for n, r in h.restypes.items() if r is not C.c_int} == {"stl_person_boxes_workspace"}
    assert h.restypes["stl_person_boxes_workspace"] is C.c_int64 and h.constants == {} and h.structs == {}
    assert not set(h.signatures) & set(capi.SIGNATURES)
