"""``torch.library`` registration of the hot-path kernels (namespace ``stlpose``).

SURVEY.md 8(b) / BASELINE north_star name PyTorch-ROCm custom ops as the mechanism through which the Python
host reaches the HIP kernels.  Every op below is a thin dispatcher-visible wrapper around ONE entry point of the
C ABI (``include/stlpose_hip.h`` -> ``libstlpose_hip.so``): tensors are allocated by torch, the kernel is
enqueued on the current HIP stream, nothing is computed by ATen.  There is no CPU implementation: on a CPU
tensor the dispatcher raises (no kernel registered for that backend).  Fake (meta) implementations make the ops
traceable.  The stateful whole-network ops (``stlpose::hrnet_forward`` / ``hrnet_backward`` / ``hrnet_backward_input``) take
the handle of a planned engine (``engine.Engine``), because their plans own the activation buffers.  ``flip_merge`` has an
autograd formula (``flip_merge_backward``, the kernel's adjoint).
"""
from __future__ import annotations

import weakref
from typing import Optional, Tuple

import torch

from . import capi

_LIB = torch.library.Library("stlpose", "DEF")
_ENGINES = weakref.WeakValueDictionary()   # handle -> Engine (whole-network ops); the model owns its engines


def _st() -> int:
    return torch.cuda.current_stream().cuda_stream


def _define(schema: str, fn, fake=None):
    _LIB.define(schema)
    name = schema.split("(")[0]
    _LIB.impl(name, fn, "CUDA")
    if fake is not None:
        torch.library.register_fake(f"stlpose::{name}", fake, lib=_LIB)


# ------------------------------------------------------------------ loss (reference lib/loss.py:71-94)
def _mse(output: torch.Tensor, target: torch.Tensor, weight: torch.Tensor, scale: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    o, t = output.contiguous().float(), target.contiguous().float()
    b, j = o.shape[:2]
    w = weight.float().reshape(b, j).contiguous()
    dout = torch.empty_like(o)
    partial = torch.empty(256, dtype=torch.float64, device=o.device)
    loss = torch.empty((), dtype=torch.float32, device=o.device)
    capi.call("stl_mse_loss", o.data_ptr(), t.data_ptr(), w.data_ptr(), dout.data_ptr(), partial.data_ptr(), 256, loss.data_ptr(),
              b, j, o[0, 0].numel(), float(scale), _st())
    return loss, dout


_define("person_mse(Tensor output, Tensor target, Tensor weight, float scale=1.0) -> (Tensor, Tensor)", _mse,
        lambda o, t, w, scale=1.0: (o.new_empty(()), torch.empty_like(o)))


# ------------------------------------------------------------------ decode (lib/pose_parsing.py:16-92, lib/transforms.py:147-164)
def _argmax(hm: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    hm = hm.contiguous().float()
    b, j, h, w = hm.shape
    idx = torch.empty(b, j, dtype=torch.int32, device=hm.device)
    mx = torch.empty(b, j, 1, dtype=torch.float32, device=hm.device)
    preds = torch.empty(b, j, 2, dtype=torch.float32, device=hm.device)
    capi.call("stl_heatmap_argmax", hm.data_ptr(), idx.data_ptr(), mx.data_ptr(), preds.data_ptr(), b * j, h, w, _st())
    return idx, mx, preds


_define("heatmap_argmax(Tensor heatmaps) -> (Tensor, Tensor, Tensor)", _argmax,
        lambda hm: (hm.new_empty(hm.shape[:2], dtype=torch.int32), hm.new_empty(*hm.shape[:2], 1), hm.new_empty(*hm.shape[:2], 2)))


def _final_preds(hm: torch.Tensor, center: torch.Tensor, scale: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    hm = hm.contiguous().float()
    b, j, h, w = hm.shape
    preds = torch.empty(b, j, 2, dtype=torch.float32, device=hm.device)
    mx = torch.empty(b, j, 1, dtype=torch.float32, device=hm.device)
    capi.call("stl_final_preds", hm.data_ptr(), center.contiguous().float().data_ptr(), scale.contiguous().float().data_ptr(),
              preds.data_ptr(), mx.data_ptr(), b, j, h, w, _st())
    return preds, mx


_define("final_preds(Tensor heatmaps, Tensor center, Tensor scale) -> (Tensor, Tensor)", _final_preds,
        lambda hm, c, s: (hm.new_empty(*hm.shape[:2], 2), hm.new_empty(*hm.shape[:2], 1)))


def _flip_merge(out: torch.Tensor, out_flipped: torch.Tensor, perm: torch.Tensor) -> torch.Tensor:
    a, f = out.contiguous().float(), out_flipped.contiguous().float()
    r = torch.empty_like(a)
    b, j, h, w = a.shape
    capi.call("stl_flip_merge", a.data_ptr(), f.data_ptr(), r.data_ptr(), perm.to(torch.int32).contiguous().data_ptr(), b, j, h, w, _st())
    return r


_define("flip_merge(Tensor out, Tensor out_flipped, Tensor perm) -> Tensor", _flip_merge, lambda a, f, p: torch.empty_like(a))


def _flip_merge_bwd(grad: torch.Tensor, perm: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    g = grad.contiguous().float()
    da, dbf = torch.empty_like(g), torch.empty_like(g)
    b, j, h, w = g.shape
    capi.call("stl_flip_merge_backward", g.data_ptr(), da.data_ptr(), dbf.data_ptr(), perm.to(torch.int32).contiguous().data_ptr(),
              b, j, h, w, _st())
    return da, dbf


_define("flip_merge_backward(Tensor grad, Tensor perm) -> (Tensor, Tensor)", _flip_merge_bwd,
        lambda g, p: (torch.empty_like(g, dtype=torch.float32), torch.empty_like(g, dtype=torch.float32)))


def _flip_merge_setup(ctx, inputs, output):
    ctx.perm = inputs[2]


def _flip_merge_autograd(ctx, grad):
    da, dbf = torch.ops.stlpose.flip_merge_backward(grad, ctx.perm)
    return da, dbf, None


torch.library.register_autograd("stlpose::flip_merge", _flip_merge_autograd, setup_context=_flip_merge_setup, lib=_LIB)


# ------------------------------------------------------------------ evaluation tail (eval_tail.py: the epoch tables)
def _f32_table(op: str, name: str, t: torch.Tensor, rows: int, tail: tuple, dtype=torch.float32) -> None:
    if t.dtype != dtype or not t.is_contiguous() or t.dim() != 1 + len(tail) or tuple(t.shape[1:]) != tail or t.shape[0] < rows:
        raise ValueError(f"stlpose {op}: {name} must be a contiguous {dtype} [>= {rows}, {', '.join(map(str, tail))}] table, got "
                         f"{t.dtype} {tuple(t.shape)}")


def _eval_tail(out: torch.Tensor, out_flipped: Optional[torch.Tensor], perm: torch.Tensor, target: torch.Tensor, target_weight: torch.Tensor,
               pred_xy: torch.Tensor, tgt_xy: torch.Tensor, coords: torch.Tensor, maxval: torch.Tensor, partial: torch.Tensor,
               losses: torch.Tensor, row0: int, slot: int) -> None:
    """Two launches, no allocation of results and no sync: stl_eval_tail into rows row0.. of the tables and into partial [B * J],
    stl_sum_partials of those into losses[slot]."""
    op = "eval_tail"
    a, t = out.contiguous().float(), target.contiguous().float()
    f = out_flipped.contiguous().float() if out_flipped is not None else None
    if a.dim() != 4 or t.shape != a.shape or (f is not None and f.shape != a.shape):
        raise ValueError(f"stlpose {op}: out {tuple(out.shape)}, out_flipped {None if f is None else tuple(f.shape)} and target "
                         f"{tuple(target.shape)} must be one [B, J, H, W]")
    b, j, h, w = a.shape
    if target_weight.numel() != b * j:
        raise ValueError(f"stlpose {op}: target_weight {tuple(target_weight.shape)} for {b} x {j} maps")
    if perm.numel() != j:
        raise ValueError(f"stlpose {op}: perm of {perm.numel()} entries for {j} joints")
    if row0 < 0 or slot < 0 or slot >= losses.numel() or losses.dtype != torch.float32 or not losses.is_contiguous():
        raise ValueError(f"stlpose {op}: row0 {row0}, slot {slot} of a float32 loss table of {losses.numel()}")
    for name, tab, tail in (("pred_xy", pred_xy, (j, 2)), ("tgt_xy", tgt_xy, (j, 2)), ("coords", coords, (j, 2)), ("maxval", maxval, (j,))):
        _f32_table(op, name, tab, row0 + b, tail)
    if partial.dtype != torch.float64 or not partial.is_contiguous() or partial.numel() < b * j:
        raise ValueError(f"stlpose {op}: partial must be contiguous float64 with at least {b * j} entries")
    if b * j == 0:
        return
    tw = target_weight.float().reshape(b, j).contiguous()
    p = perm.to(torch.int32).contiguous()
    capi.call("stl_eval_tail", a.data_ptr(), f.data_ptr() if f is not None else None, p.data_ptr(), t.data_ptr(), tw.data_ptr(),
              pred_xy.data_ptr(), tgt_xy.data_ptr(), coords.data_ptr(), maxval.data_ptr(), partial.data_ptr(), b, j, h, w, row0, _st())
    capi.call("stl_sum_partials", partial.data_ptr(), b * j, 0.5 / float(b * j * h * w), losses.data_ptr() + 4 * slot, 0, _st())


_define("eval_tail(Tensor out, Tensor? out_flipped, Tensor perm, Tensor target, Tensor target_weight, Tensor(a!) pred_xy, "
        "Tensor(b!) tgt_xy, Tensor(c!) coords, Tensor(d!) maxval, Tensor(e!) partial, Tensor(f!) losses, int row0, int slot) -> ()",
        _eval_tail, lambda *a: None)


def _eval_affine(coords: torch.Tensor, maxval: torch.Tensor, center: torch.Tensor, scale: torch.Tensor, h: int, w: int) -> torch.Tensor:
    op = "eval_affine"
    n = center.shape[0]
    if coords.dim() != 3 or coords.shape[2] != 2:
        raise ValueError(f"stlpose {op}: coords {tuple(coords.shape)} ([>= N, J, 2])")
    j = coords.shape[1]
    _f32_table(op, "coords", coords, n, (j, 2))
    _f32_table(op, "maxval", maxval, n, (j,))
    if tuple(center.shape) != (n, 2) or tuple(scale.shape) != (n, 2):
        raise ValueError(f"stlpose {op}: center {tuple(center.shape)} and scale {tuple(scale.shape)} must be [N, 2]")
    c, s = center.contiguous().float(), scale.contiguous().float()
    preds = torch.empty(n, j, 3, dtype=torch.float32, device=coords.device)
    capi.call("stl_eval_affine", coords.data_ptr(), maxval.data_ptr(), c.data_ptr(), s.data_ptr(), preds.data_ptr(), n, j, h, w, _st())
    return preds


_define("eval_affine(Tensor coords, Tensor maxval, Tensor center, Tensor scale, int h, int w) -> Tensor", _eval_affine,
        lambda co, mv, c, s, h, w: co.new_empty(c.shape[0], co.shape[1], 3))


# ------------------------------------------------------------------ data pipeline (data/JointsDataset.py:189-286)
def _targets(joints: torch.Tensor, vis: torch.Tensor, hh: int, wh: int, sx: float, sy: float, sigma: float) -> Tuple[torch.Tensor, torch.Tensor]:
    j, v = joints.contiguous().float(), vis.contiguous().float()
    b, nj = j.shape[:2]
    target = torch.empty(b, nj, hh, wh, dtype=torch.float32, device=j.device)
    tw = torch.empty(b, nj, dtype=torch.float32, device=j.device)
    capi.call("stl_gaussian_targets", j.data_ptr(), v.data_ptr(), target.data_ptr(), tw.data_ptr(), b, nj, hh, wh, float(sx), float(sy),
              float(sigma), _st())
    return target, tw


_define("gaussian_targets(Tensor joints, Tensor vis, int hh, int wh, float sx, float sy, float sigma) -> (Tensor, Tensor)", _targets,
        lambda j, v, hh, wh, sx, sy, sigma: (j.new_empty(j.shape[0], j.shape[1], hh, wh), j.new_empty(j.shape[0], j.shape[1])))


def _crop(src: torch.Tensor, src_off: torch.Tensor, src_hw: torch.Tensor, minv: torch.Tensor, flip: torch.Tensor, ho: int, wo: int,
          mean: torch.Tensor, std: torch.Tensor) -> torch.Tensor:
    b = src_hw.shape[0]
    out = torch.empty(b, 3, ho, wo, dtype=torch.float32, device=src.device)
    capi.call("stl_affine_crop", src.data_ptr(), src_off.data_ptr(), src_hw.data_ptr(), minv.data_ptr(), flip.data_ptr(), out.data_ptr(),
              b, ho, wo, mean.data_ptr(), std.data_ptr(), _st())
    return out


_define("affine_crop(Tensor src, Tensor src_off, Tensor src_hw, Tensor minv, Tensor flip, int ho, int wo, Tensor mean, Tensor std) -> Tensor",
        _crop, lambda s, o, hw, m, f, ho, wo, mean, std: s.new_empty(hw.shape[0], 3, ho, wo, dtype=torch.float32))


def _pose_augment(joints_tab, vis_tab, center_tab, scale_tab, width_tab, index, draws, train: bool, flip_enabled: bool, scale_factor: float,
                  rot_factor: float, num_joints_half_body: int, prob_half_body: float, wo: int, ho: int):
    """One launch of stl_pose_augment; every shape, dtype and device the kernel relies on is checked here, nothing is read back."""
    op = "pose_augment"
    j = capi.POSE_JOINTS
    if joints_tab.dim() != 3 or tuple(joints_tab.shape[1:]) != (j, 3):
        raise ValueError(f"stlpose {op}: joints must be [N, {j}, 3]; the kernel's flip pairs and upper-body ids are COCO's {j} joints, got "
                         f"{tuple(joints_tab.shape)}")
    n = _table(op, "joints", joints_tab, torch.float64, "N", tail=(j, 3))
    if n < 1:
        raise ValueError(f"stlpose {op}: an empty person table")
    _table(op, "joints_vis", vis_tab, torch.float64, "N", n, tail=(j, 3))
    _table(op, "center", center_tab, torch.float32, "N", n, tail=(2,))
    _table(op, "scale", scale_tab, torch.float32, "N", n, tail=(2,))
    _table(op, "width", width_tab, torch.int32, "N", n)
    b = _table(op, "index", index, torch.int64, "B")
    _table(op, "draws", draws, torch.float64, "B", b, tail=(6,))
    if not joints_tab.is_cuda:
        raise RuntimeError(f"stlpose {op}: the person tables must be on the GPU")
    dev = joints_tab.device
    tabs = (("joints_vis", vis_tab), ("center", center_tab), ("scale", scale_tab), ("width", width_tab), ("index", index), ("draws", draws))
    _same_device(tabs, dev)
    for name, t in (("joints", joints_tab),) + tabs:
        if not t.is_contiguous():
            raise ValueError(f"stlpose {op}: {name} must be contiguous")
    if wo < 1 or ho < 1 or scale_factor < 0 or rot_factor < 0:
        raise ValueError(f"stlpose {op}: crop {wo} x {ho}, scale_factor {scale_factor}, rot_factor {rot_factor}")
    f64 = dict(dtype=torch.float64, device=dev)
    out = (torch.empty(b, 2, **f64), torch.empty(b, 2, **f64), torch.empty(b, **f64), torch.empty(b, dtype=torch.int32, device=dev),
           torch.empty(b, 2, 3, **f64), torch.empty(b, 6, dtype=torch.float32, device=dev), torch.empty(b, j, 3, **f64),
           torch.empty(b, j, 3, **f64), torch.empty(b, j, 2, dtype=torch.float32, device=dev),
           torch.empty(b, j, dtype=torch.float32, device=dev))
    capi.call("stl_pose_augment", joints_tab.data_ptr(), vis_tab.data_ptr(), center_tab.data_ptr(), scale_tab.data_ptr(),
              width_tab.data_ptr(), n, index.data_ptr(), draws.data_ptr(), b, int(bool(train)), int(bool(flip_enabled)),
              float(scale_factor), float(rot_factor), int(num_joints_half_body), float(prob_half_body), int(wo), int(ho),
              *(t.data_ptr() for t in out), _st())
    return out


def _pose_augment_fake(jt, vt, ct, st, wt, index, draws, train, flip_enabled, sf, rf, nh, ph, wo, ho):
    b, j = index.shape[0], jt.shape[1]
    return (jt.new_empty(b, 2), jt.new_empty(b, 2), jt.new_empty(b), jt.new_empty(b, dtype=torch.int32), jt.new_empty(b, 2, 3),
            jt.new_empty(b, 6, dtype=torch.float32), jt.new_empty(b, j, 3), jt.new_empty(b, j, 3),
            jt.new_empty(b, j, 2, dtype=torch.float32), jt.new_empty(b, j, dtype=torch.float32))


# center, scale, rot, flip, trans, minv, joints, joints_vis, joints_xy (fp32), vis0 (fp32): stl_pose_augment in include/stlpose_hip.h
_define("pose_augment(Tensor joints, Tensor joints_vis, Tensor center, Tensor scale, Tensor width, Tensor index, Tensor draws, bool train, "
        "bool flip_enabled, float scale_factor, float rot_factor, int num_joints_half_body, float prob_half_body, int wo, int ho) "
        "-> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)", _pose_augment, _pose_augment_fake)


# ------------------------------------------------------------------ whole network (models/HRnet.py:433-468 + its autograd backward)
def register_engine(eng) -> int:
    h = id(eng)
    _ENGINES[h] = eng
    return h


def _hrnet_fwd(img: torch.Tensor, handle: int) -> torch.Tensor:
    eng = _ENGINES[handle]
    eng.img.copy_(img)
    eng.forward(_st())
    return eng.out.clone()


def _hrnet_bwd(grad_out: torch.Tensor, handle: int) -> torch.Tensor:
    """Backward of the planned network for the LAST forward of that plan; returns the flat parameter gradient."""
    eng = _ENGINES[handle]
    eng.dout.copy_(grad_out)
    eng.backward(_st())
    return eng.store.grads.clone()   # a fresh tensor: an op must not hand out an alias of the plan's own buffer


def _hrnet_bwd_input(grad_out: torch.Tensor, handle: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Backward of a plan built with input_grad, for the LAST forward of that plan: (flat parameter gradient, dL/d(img)).  An eval
    plan computes no parameter gradients: its first result is empty (0 elements) and store.grads is left as it was."""
    eng = _ENGINES[handle]
    assert eng.input_grad, "hrnet_backward_input: the plan was built without input_grad"
    eng.dout.copy_(grad_out)
    eng.backward(_st())
    flat = eng.store.grads.clone() if eng.training else grad_out.new_empty(0, dtype=torch.float32)
    return flat, eng.dimg.clone()


def _hrnet_fwd_fake(img, engine):
    eng = _ENGINES[engine]   # joints and output stride come from the planned engine, not from constants
    return img.new_empty(tuple(eng.out.shape), dtype=torch.float32)


def _hrnet_bwd_fake(grad_out, engine):
    return grad_out.new_empty(_ENGINES[engine].store.nparam, dtype=torch.float32)


_define("hrnet_forward(Tensor img, int engine) -> Tensor", _hrnet_fwd, _hrnet_fwd_fake)
_define("hrnet_backward(Tensor grad_out, int engine) -> Tensor", _hrnet_bwd, _hrnet_bwd_fake)


def _hrnet_bwd_input_fake(grad_out, engine):
    eng = _ENGINES[engine]
    return (grad_out.new_empty(eng.store.nparam if eng.training else 0, dtype=torch.float32),
            grad_out.new_empty((eng.B, 3, eng.H, eng.W), dtype=torch.float32))


_define("hrnet_backward_input(Tensor grad_out, int engine) -> (Tensor, Tensor)", _hrnet_bwd_input, _hrnet_bwd_input_fake)

# ------------------------------------------------------------------ pose retrieval (lib/pose_database.py, lib/metrics.py:25-149)
# method / penalization / approach travel as strings; an unknown name reaches the C ABI as -1 and is refused there.
# The C ABI sees pointers and (Q, N, D) only: every shape it relies on is checked here, before anything is launched.
def _same_device(ts, dev):
    for name, t in ts:
        if t is not None and t.device != dev:
            raise RuntimeError(f"stlpose pose op: {name} is on {t.device}, the queries on {dev}")


def _check_pose_shapes(query, conf, database, labels=None, qlabels=None):
    if query.dim() != 2 or database.dim() != 2:
        raise RuntimeError(f"stlpose pose op: query and database must be 2-D [Q, D] / [N, D], got {tuple(query.shape)} and "
                           f"{tuple(database.shape)}")
    if query.shape[1] != database.shape[1]:
        raise RuntimeError(f"stlpose pose op: query width {query.shape[1]} differs from database width {database.shape[1]}")
    if conf is not None and tuple(conf.shape) != tuple(query.shape):
        raise RuntimeError(f"stlpose pose op: confidence must have the query's shape {tuple(query.shape)}, got {tuple(conf.shape)}")
    if labels is not None:
        nl = labels.shape[0] if labels.dim() == 2 else -1
        if labels.dim() != 2 or labels.shape[1] != database.shape[0]:
            raise RuntimeError(f"stlpose pose_rank: labels must be [L, N={database.shape[0]}], got {tuple(labels.shape)}")
        if qlabels is None or tuple(qlabels.shape) != (nl, query.shape[0]):
            raise RuntimeError(f"stlpose pose_rank: qlabels must be [L={nl}, Q={query.shape[0]}], got "
                               f"{None if qlabels is None else tuple(qlabels.shape)}")
    _same_device((("database", database), ("confidence", conf), ("labels", labels), ("qlabels", qlabels)), query.device)


def _pose_args(query, conf, database, method, penalization):
    _check_pose_shapes(query, conf, database)
    q, db = query.contiguous().float(), database.contiguous().float()
    c = conf.contiguous().float() if conf is not None else None
    return q, c, db, capi.POSE_METHOD.get(method, -1), capi.POSE_PEN.get(penalization, -1)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _pose_vectors(joints: torch.Tensor, approach: str, normalize: bool) -> torch.Tensor:
    if joints.dim() != 3 or joints.shape[1] != capi.POSE_JOINTS or joints.shape[2] < 2:
        raise RuntimeError(f"stlpose pose_vectors: joints must be [N, 17, C >= 2], got {tuple(joints.shape)}")
    j = joints.contiguous().float()
    n = j.shape[0]
    out = torch.empty(n, capi.POSE_DIM.get(approach, 34), dtype=torch.float32, device=j.device)
    # row stride from the shape: a contiguous tensor may report any stride for a size-1 batch dimension
    capi.call("stl_pose_vectors", j.data_ptr(), j.shape[1] * j.shape[2], j.shape[2], out.data_ptr(), n, capi.POSE_APPROACH.get(approach, -1),
              int(normalize), _st())
    return out


_define("pose_vectors(Tensor joints, str approach, bool normalize) -> Tensor", _pose_vectors,
        lambda j, approach, normalize: j.new_empty(j.shape[0], capi.POSE_DIM.get(approach, 34), dtype=torch.float32))


def _pose_distances(query, conf, database, method: str, penalization: str) -> torch.Tensor:
    q, c, db, m, p = _pose_args(query, conf, database, method, penalization)
    out = torch.empty(q.shape[0], db.shape[0], dtype=torch.float32, device=q.device)
    capi.call("stl_pose_distances", q.data_ptr(), _ptr(c), db.data_ptr(), out.data_ptr(), q.shape[0], db.shape[0], q.shape[1], m, p,
              _st())
    return out


_define("pose_distances(Tensor query, Tensor? conf, Tensor database, str method, str penalization) -> Tensor", _pose_distances,
        lambda q, c, db, m, p: q.new_empty(q.shape[0], db.shape[0], dtype=torch.float32))


def _pose_topk(query, conf, database, method: str, penalization: str, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    q, c, db, m, p = _pose_args(query, conf, database, method, penalization)
    nq, n, d = q.shape[0], db.shape[0], q.shape[1]
    need = capi.lib().stl_pose_topk_workspace(nq, n, k, d)
    capi.check(min(need, 0), "stl_pose_topk")
    work = torch.empty(max(need, 8), dtype=torch.uint8, device=q.device)
    idx = torch.empty(nq, k, dtype=torch.int64, device=q.device)
    dist = torch.empty(nq, k, dtype=torch.float32, device=q.device)
    capi.call("stl_pose_topk", q.data_ptr(), _ptr(c), db.data_ptr(), nq, n, d, m, p, k, idx.data_ptr(), dist.data_ptr(), work.data_ptr(),
              work.numel(), _st())
    return idx, dist


_define("pose_topk(Tensor query, Tensor? conf, Tensor database, str method, str penalization, int k) -> (Tensor, Tensor)", _pose_topk,
        lambda q, c, db, m, p, k: (q.new_empty(q.shape[0], k, dtype=torch.int64), q.new_empty(q.shape[0], k, dtype=torch.float32)))


def _pose_rank(query, conf, database, method: str, penalization: str, k_out: int, labels, qlabels, k_eff: int):
    _check_pose_shapes(query, conf, database, labels, qlabels)
    q, c, db, m, p = _pose_args(query, conf, database, method, penalization)
    nq, n, d = q.shape[0], db.shape[0], q.shape[1]
    idx = torch.empty(nq, k_out, dtype=torch.int64, device=q.device)
    dist = torch.empty(nq, k_out, dtype=torch.float32, device=q.device)
    lab = labels.contiguous().to(torch.int32) if labels is not None else None
    qlab = qlabels.contiguous().to(torch.int32) if qlabels is not None else None
    nl = lab.shape[0] if lab is not None else 0
    scores = torch.empty(nq, nl, capi.POSE_NSCORES, dtype=torch.float64, device=q.device)
    capi.call("stl_pose_rank", q.data_ptr(), _ptr(c), db.data_ptr(), nq, n, d, m, p, k_out, idx.data_ptr(), dist.data_ptr(), _ptr(lab),
              _ptr(qlab), nl, k_eff, scores.data_ptr(), _st())
    return idx, dist, scores


def _pose_rank_fake(q, c, db, m, p, k_out, labels, qlabels, k_eff):
    nl = labels.shape[0] if labels is not None else 0
    return (q.new_empty(q.shape[0], k_out, dtype=torch.int64), q.new_empty(q.shape[0], k_out, dtype=torch.float32),
            q.new_empty(q.shape[0], nl, capi.POSE_NSCORES, dtype=torch.float64))


_define("pose_rank(Tensor query, Tensor? conf, Tensor database, str method, str penalization, int k_out, Tensor? labels, "
        "Tensor? qlabels, int k_eff) -> (Tensor, Tensor, Tensor)", _pose_rank, _pose_rank_fake)


def _pose_rank_any(query, conf, database, method: str, penalization: str, k_out: int, labels, qlabels, k_eff: int):
    """pose_rank at any N <= capi.POSE_RANK_ANY_MAX; the workspace (two [Q, N] key arrays above N = POSE_RANK_MAX) is allocated here."""
    _check_pose_shapes(query, conf, database, labels, qlabels)
    q, c, db, m, p = _pose_args(query, conf, database, method, penalization)
    nq, n, d = q.shape[0], db.shape[0], q.shape[1]
    need = capi.lib().stl_pose_rank_any_workspace(nq, n)
    capi.check(min(need, 0), "stl_pose_rank_any")
    work = torch.empty(need, dtype=torch.uint8, device=q.device)
    idx = torch.empty(nq, k_out, dtype=torch.int64, device=q.device)
    dist = torch.empty(nq, k_out, dtype=torch.float32, device=q.device)
    lab = labels.contiguous().to(torch.int32) if labels is not None else None
    qlab = qlabels.contiguous().to(torch.int32) if qlabels is not None else None
    nl = lab.shape[0] if lab is not None else 0
    scores = torch.empty(nq, nl, capi.POSE_NSCORES, dtype=torch.float64, device=q.device)
    capi.call("stl_pose_rank_any", q.data_ptr(), _ptr(c), db.data_ptr(), nq, n, d, m, p, k_out, idx.data_ptr(), dist.data_ptr(),
              _ptr(lab), _ptr(qlab), nl, k_eff, scores.data_ptr(), work.data_ptr(), work.numel(), _st())
    return idx, dist, scores


_define("pose_rank_any(Tensor query, Tensor? conf, Tensor database, str method, str penalization, int k_out, Tensor? labels, "
        "Tensor? qlabels, int k_eff) -> (Tensor, Tensor, Tensor)", _pose_rank_any, _pose_rank_fake)

# ------------------------------------------------------------------ top-down extraction (lib/bounding_box.py, lib/pose_parsing.py)
# Every shape, dtype, device and cap the kernels rely on is checked here, before anything is launched.
def _box_select(boxes, scores, labels, offsets, label: int, score_thr: Optional[float], iou_thr: float) -> Tuple[torch.Tensor, torch.Tensor]:
    if boxes.dim() != 2 or boxes.shape[1] != 4 or boxes.dtype != torch.float32:
        raise ValueError(f"stlpose box_select: boxes must be float32 [N, 4], got {boxes.dtype} {tuple(boxes.shape)}")
    n = boxes.shape[0]
    if scores.dim() != 1 or scores.shape[0] != n or scores.dtype != torch.float32:
        raise ValueError(f"stlpose box_select: scores must be float32 [N={n}], got {scores.dtype} {tuple(scores.shape)}")
    if labels is not None and (labels.dim() != 1 or labels.shape[0] != n or labels.dtype != torch.int64):
        raise ValueError(f"stlpose box_select: labels must be int64 [N={n}], got {labels.dtype} {tuple(labels.shape)}")
    if offsets.dim() != 1 or offsets.shape[0] < 1 or offsets.dtype != torch.int64:
        raise ValueError(f"stlpose box_select: offsets must be int64 [I + 1], got {offsets.dtype} {tuple(offsets.shape)}")
    off = offsets.cpu()
    per = off[1:] - off[:-1]
    if int(off[0]) != 0 or int(off[-1]) != n or bool((per < 0).any()):
        raise ValueError(f"stlpose box_select: offsets must rise from 0 to N = {n}")
    max_n = int(per.max()) if per.numel() else 0
    if max_n > capi.BOX_MAX:
        raise ValueError(f"stlpose box_select: an image has {max_n} boxes; the cap is {capi.BOX_MAX} (STL_BOX_MAX) per image")
    if not boxes.is_cuda:
        raise RuntimeError("stlpose box_select: boxes must be on the GPU")
    _same_device((("scores", scores), ("labels", labels)), boxes.device)
    ni = per.numel()
    keep = torch.empty(n, dtype=torch.int32, device=boxes.device)
    count = torch.empty(ni, dtype=torch.int32, device=boxes.device)
    b, s = boxes.contiguous(), scores.contiguous()
    lab = labels.contiguous() if labels is not None else None
    o = off.to(boxes.device)
    capi.call("stl_box_select", b.data_ptr(), s.data_ptr(), _ptr(lab), o.data_ptr(), ni, n, max_n, int(label),
              int(score_thr is not None), float(score_thr) if score_thr is not None else 0.0, float(iou_thr), keep.data_ptr(),
              count.data_ptr(), _st())
    return keep, count


_define("box_select(Tensor boxes, Tensor scores, Tensor? labels, Tensor offsets, int label, float? score_thr, float iou_thr) "
        "-> (Tensor, Tensor)", _box_select,
        lambda b, s, l, o, label, st, it: (b.new_empty(b.shape[0], dtype=torch.int32), b.new_empty(o.shape[0] - 1, dtype=torch.int32)))


def _resize_argmax(heatmaps: torch.Tensor, ho: int, wo: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    if heatmaps.dim() != 4 or heatmaps.dtype != torch.float32:
        raise ValueError(f"stlpose heatmap_resize_argmax: heatmaps must be float32 [B, J, H, W], got {heatmaps.dtype} "
                         f"{tuple(heatmaps.shape)}")
    b, j, h, w = heatmaps.shape
    if h * w > capi.RESIZE_SRC_MAX or h < 1 or w < 1:
        raise ValueError(f"stlpose heatmap_resize_argmax: a {h} x {w} map; the cap is H * W <= {capi.RESIZE_SRC_MAX}")
    if not (1 <= ho <= capi.RESIZE_DST_MAX and 1 <= wo <= capi.RESIZE_DST_MAX):
        raise ValueError(f"stlpose heatmap_resize_argmax: output {ho} x {wo}; each side must be in 1 .. {capi.RESIZE_DST_MAX}")
    if not heatmaps.is_cuda:
        raise RuntimeError("stlpose heatmap_resize_argmax: heatmaps must be on the GPU")
    hm = heatmaps.contiguous()
    idx = torch.empty(b, j, dtype=torch.int32, device=hm.device)
    mx = torch.empty(b, j, dtype=torch.float32, device=hm.device)
    preds = torch.empty(b, j, 2, dtype=torch.float32, device=hm.device)
    capi.call("stl_heatmap_resize_argmax", hm.data_ptr(), b * j, h, w, int(ho), int(wo), idx.data_ptr(), mx.data_ptr(), preds.data_ptr(),
              _st())
    return idx, mx, preds


_define("heatmap_resize_argmax(Tensor heatmaps, int ho, int wo) -> (Tensor, Tensor, Tensor)", _resize_argmax,
        lambda hm, ho, wo: (hm.new_empty(hm.shape[:2], dtype=torch.int32), hm.new_empty(hm.shape[:2]), hm.new_empty(*hm.shape[:2], 2)))

# ------------------------------------------------------------------ detector postprocess (efficientdet_utils/utils.py:150-187)
def _det_decode(reg, cls, anchors, threshold: float, xmax: float, ymax: float):
    if reg.dim() != 3 or reg.shape[2] != 4 or reg.dtype != torch.float32:
        raise ValueError(f"stlpose det_decode: regression must be float32 [B, A, 4], got {reg.dtype} {tuple(reg.shape)}")
    b, a = reg.shape[:2]
    if cls.dim() != 3 or tuple(cls.shape[:2]) != (b, a) or cls.shape[2] < 1 or cls.dtype != torch.float32:
        raise ValueError(f"stlpose det_decode: classification must be float32 [B={b}, A={a}, nc], got {cls.dtype} {tuple(cls.shape)}")
    if tuple(anchors.shape[-2:]) != (a, 4) or anchors.numel() != a * 4 or anchors.dtype != torch.float32:
        raise ValueError(f"stlpose det_decode: anchors must be float32 [A={a}, 4], got {anchors.dtype} {tuple(anchors.shape)}")
    if not reg.is_cuda:
        raise RuntimeError("stlpose det_decode: regression must be on the GPU")
    _same_device((("classification", cls), ("anchors", anchors)), reg.device)
    r, c, an = reg.contiguous(), cls.contiguous(), anchors.contiguous()
    boxes = torch.empty(b, a, 4, device=reg.device)
    scores = torch.empty(b, a, device=reg.device)
    classes = torch.empty(b, a, dtype=torch.int32, device=reg.device)
    index = torch.empty(b, a, dtype=torch.int32, device=reg.device)
    count = torch.empty(b, dtype=torch.int32, device=reg.device)
    capi.call("stl_det_decode", r.data_ptr(), c.data_ptr(), an.data_ptr(), b, a, c.shape[2], float(threshold), float(xmax), float(ymax),
              boxes.data_ptr(), scores.data_ptr(), classes.data_ptr(), index.data_ptr(), count.data_ptr(), _st())
    return boxes, scores, classes, index, count


_define("det_decode(Tensor regression, Tensor classification, Tensor anchors, float threshold, float xmax, float ymax) "
        "-> (Tensor, Tensor, Tensor, Tensor, Tensor)", _det_decode,
        lambda r, c, a, t, xm, ym: (r.new_empty(r.shape), r.new_empty(r.shape[:2]), r.new_empty(r.shape[:2], dtype=torch.int32),
                                    r.new_empty(r.shape[:2], dtype=torch.int32), r.new_empty(r.shape[0], dtype=torch.int32)))


def _det_nms(boxes, classes, order, iou_thr: float):
    if boxes.dim() != 2 or boxes.shape[1] != 4 or boxes.dtype != torch.float32:
        raise ValueError(f"stlpose det_nms: boxes must be float32 [n, 4], got {boxes.dtype} {tuple(boxes.shape)}")
    n = boxes.shape[0]
    if n > capi.DET_NMS_MAX:
        raise ValueError(f"stlpose det_nms: {n} candidates; the cap is {capi.DET_NMS_MAX} (STL_DET_NMS_MAX)")
    for name, t in (("classes", classes), ("order", order)):
        if t.dim() != 1 or t.shape[0] != n or t.dtype != torch.int32:
            raise ValueError(f"stlpose det_nms: {name} must be int32 [n={n}], got {t.dtype} {tuple(t.shape)}")
    if not boxes.is_cuda:
        raise RuntimeError("stlpose det_nms: boxes must be on the GPU")
    _same_device((("classes", classes), ("order", order)), boxes.device)
    keep = torch.empty(n, dtype=torch.int32, device=boxes.device)
    count = torch.empty(1, dtype=torch.int32, device=boxes.device)
    work = torch.empty(max(1, int(capi.lib().stl_det_nms_workspace(n))), dtype=torch.uint8, device=boxes.device)
    b, c, o = boxes.contiguous(), classes.contiguous(), order.contiguous()
    capi.call("stl_det_nms", b.data_ptr(), c.data_ptr(), o.data_ptr(), n, float(iou_thr), work.data_ptr(), keep.data_ptr(),
              count.data_ptr(), _st())
    return keep, count


_define("det_nms(Tensor boxes, Tensor classes, Tensor order, float iou_thr) -> (Tensor, Tensor)", _det_nms,
        lambda b, c, o, t: (b.new_empty(b.shape[0], dtype=torch.int32), b.new_empty(1, dtype=torch.int32)))


# ------------------------------------------------------------------ detector fine-tuning loss (csrc/detector_train.hip)
def _det_loss(reg, cls, anchors, gt, offsets, alpha: float, gamma: float, box_weight: float):
    if reg.dim() != 3 or reg.shape[2] != 4 or reg.dtype != torch.float32 or reg.shape[0] < 1 or reg.shape[1] < 1:
        raise ValueError(f"stlpose det_loss: regression must be float32 [B, A, 4], got {reg.dtype} {tuple(reg.shape)}")
    b, a = reg.shape[:2]
    if cls.dim() != 3 or tuple(cls.shape[:2]) != (b, a) or cls.shape[2] < 1 or cls.dtype != torch.float32:
        raise ValueError(f"stlpose det_loss: classification must be float32 [B={b}, A={a}, nc], got {cls.dtype} {tuple(cls.shape)}")
    if tuple(anchors.shape[-2:]) != (a, 4) or anchors.numel() != a * 4 or anchors.dtype != torch.float32:
        raise ValueError(f"stlpose det_loss: anchors must be float32 [A={a}, 4], got {anchors.dtype} {tuple(anchors.shape)}")
    if gt.dim() != 2 or gt.shape[1] != 5 or gt.dtype != torch.float32:
        raise ValueError(f"stlpose det_loss: gt must be float32 [sum G, 5] (x1, y1, x2, y2, class), got {gt.dtype} {tuple(gt.shape)}")
    if offsets.dim() != 1 or offsets.shape[0] != b + 1 or offsets.dtype != torch.int32:
        raise ValueError(f"stlpose det_loss: offsets must be int32 [B + 1 = {b + 1}], got {offsets.dtype} {tuple(offsets.shape)}")
    if not (0.0 <= alpha <= 1.0) or gamma < 1.0:
        raise ValueError(f"stlpose det_loss: alpha {alpha} (0 .. 1), gamma {gamma} (>= 1)")
    if not reg.is_cuda:
        raise RuntimeError("stlpose det_loss: regression must be on the GPU")
    _same_device((("classification", cls), ("anchors", anchors), ("gt", gt), ("offsets", offsets)), reg.device)
    r, c, an, g, o = reg.contiguous(), cls.contiguous(), anchors.contiguous(), gt.contiguous(), offsets.contiguous()
    nc = c.shape[2]
    losses = torch.empty(2, device=reg.device)
    dreg, dlogit = torch.empty_like(r), torch.empty_like(c)
    npos = torch.empty(b, dtype=torch.int32, device=reg.device)
    assign = torch.empty(b, a, dtype=torch.int32, device=reg.device)
    per_image = torch.empty(b, 2, device=reg.device)
    capi.call("stl_det_loss", r.data_ptr(), c.data_ptr(), an.data_ptr(), g.data_ptr() if g.numel() else None, o.data_ptr(), b, a, nc,
              float(alpha), float(gamma), float(box_weight), assign.data_ptr(), per_image.data_ptr(), losses.data_ptr(),
              dreg.data_ptr(), dlogit.data_ptr(), npos.data_ptr(), _st())
    return losses, dreg, dlogit, npos


# losses [2] = (classification, regression); the offsets must be ascending from 0 to gt.shape[0] and the classes inside [0, nc)
# (EfficientDetBackbone.detection_loss builds them from validated targets)
_define("det_loss(Tensor regression, Tensor classification, Tensor anchors, Tensor gt, Tensor offsets, float alpha, float gamma, "
        "float box_weight) -> (Tensor, Tensor, Tensor, Tensor)", _det_loss,
        lambda r, c, a, g, o, al, ga, bw: (r.new_empty(2), r.new_empty(r.shape), c.new_empty(c.shape),
                                           r.new_empty(r.shape[0], dtype=torch.int32)))

# ------------------------------------------------------------------ COCO box AP (csrc/box_ap.hip, csrc/coco_match.inc; COCOeval "bbox")
# Every shape, dtype, device and cap the kernels rely on is checked here, before anything is launched.
class BoxApCapError(ValueError):
    """A cap of box_ap_match is exceeded.  ``image_index`` is the image's position in the ragged tables: the op knows no image ids
    (detection_eval re-raises with the id)."""

    def __init__(self, message: str, image_index: int):
        super().__init__(message)
        self.image_index = image_index


def _ragged(op: str, name: str, offsets, n: int):
    """offsets int64 [I + 1] rising from 0 to n, as a CPU tensor; the rows per image."""
    if offsets.dim() != 1 or offsets.shape[0] < 1 or offsets.dtype != torch.int64:
        raise ValueError(f"stlpose {op}: {name} must be int64 [I + 1], got {offsets.dtype} {tuple(offsets.shape)}")
    off = offsets.cpu()
    per = off[1:] - off[:-1]
    if int(off[0]) != 0 or int(off[-1]) != n or bool((per < 0).any()):
        raise ValueError(f"stlpose {op}: {name} must rise from 0 to {n}")
    return off, per


def _doubles(v):
    return (capi.C.c_double * len(v))(*[float(x) for x in v])


def _table(op: str, name: str, t, dtype, rows: str, n=None, tail=(), note: str = "") -> int:
    """t must be `dtype` [rows, *tail] with n rows (None: any number); its row count."""
    if t.dim() != 1 + len(tail) or tuple(t.shape[1:]) != tuple(tail) or (n is not None and t.shape[0] != n) or t.dtype != dtype:
        dims = ", ".join([rows if n is None else f"{rows}={n}"] + [str(d) for d in tail])
        raise ValueError(f"stlpose {op}: {name} must be {str(dtype).removeprefix('torch.')} [{dims}]{note}, got {t.dtype} {tuple(t.shape)}")
    return t.shape[0]


def _match_images(op: str, n: int, g: int, det_offsets, gt_offsets, thrs, area_ranges, metric: str, num_thrs: int, num_areas: int):
    """The checks box_ap_match and oks_ap_match share once their tables have the right shapes: both offsets over the same images,
    the threshold and area-range counts, the detection cap.  Returns (det_offsets, gt_offsets) on the CPU, the ground truths per
    image and the largest detection count."""
    doff, dper = _ragged(op, "det_offsets", det_offsets, n)
    goff, gper = _ragged(op, "gt_offsets", gt_offsets, g)
    ni = dper.numel()
    if gper.numel() != ni:
        raise ValueError(f"stlpose {op}: det_offsets cover {ni} images, gt_offsets {gper.numel()}")
    if len(thrs) != num_thrs or len(area_ranges) != 2 * num_areas:
        raise ValueError(f"stlpose {op}: {num_thrs} {metric} thresholds and {num_areas} (lo, hi) area ranges, got "
                         f"{len(thrs)} and {len(area_ranges)} numbers")
    max_n = int(dper.max()) if ni else 0
    if max_n > capi.BOX_MAX:
        raise BoxApCapError(f"stlpose {op}: the image at table position {int(dper.argmax())} has {max_n} detections; the cap is "
                            f"{capi.BOX_MAX} (STL_BOX_MAX) per image", int(dper.argmax()))
    return doff, goff, gper, max_n


def _match_slots(op: str, name: str, det, scores, others, ni: int, nk: int, num_areas: int):
    """The last checks (no NaN score, everything on the GPU of `det`, the table called `name`) and the six outputs of a match op."""
    if bool(torch.isnan(scores).any()):
        raise ValueError(f"stlpose {op}: a score is NaN")
    if not det.is_cuda:
        raise RuntimeError(f"stlpose {op}: {name} must be on the GPU")
    dev, n = det.device, det.shape[0]
    _same_device((("scores", scores),) + tuple(others), dev)
    return (torch.zeros(n, dtype=scores.dtype, device=dev),            # slot_score
            torch.full((n,), -1, dtype=torch.int32, device=dev),       # slot_cat: rows no workgroup claims stay out of every category
            torch.zeros(n, dtype=torch.int32, device=dev),             # slot_rank
            torch.zeros(n, dtype=torch.int64, device=dev),             # matched
            torch.zeros(n, dtype=torch.int64, device=dev),             # ignored
            torch.empty(ni, nk, num_areas, dtype=torch.int32, device=dev))   # npig


def _box_ap_match(boxes, scores, labels, det_offsets, gt_boxes, gt_area, gt_label, gt_crowd, gt_offsets, categories, iou_thrs, area_ranges):
    op = "box_ap_match"
    n = _table(op, "boxes", boxes, torch.float64, "N", tail=(4,), note=" (x, y, w, h)")
    _table(op, "scores", scores, torch.float32, "N", n)
    _table(op, "labels", labels, torch.int64, "N", n)
    g = _table(op, "gt_boxes", gt_boxes, torch.float64, "G", tail=(4,), note=" (x, y, w, h)")
    for name, t, dt in (("gt_area", gt_area, torch.float64), ("gt_label", gt_label, torch.int64), ("gt_crowd", gt_crowd, torch.uint8)):
        if t.dim() != 1 or t.shape[0] != g or t.dtype != dt:
            raise ValueError(f"stlpose {op}: {name} must be {dt} [G={g}], got {t.dtype} {tuple(t.shape)}")
    nk = _table(op, "categories", categories, torch.int64, "K")
    cats = categories.cpu()
    if nk > 65535 or bool((cats[1:] <= cats[:-1]).any()):
        raise ValueError(f"stlpose {op}: categories must be strictly ascending, at most 65535 of them")
    doff, goff, gper, max_n = _match_images(op, n, g, det_offsets, gt_offsets, iou_thrs, area_ranges, "IoU", capi.BOX_AP_THRS,
                                            capi.BOX_AP_AREAS)
    ni, max_g = gper.numel(), 0
    if g and nk:   # ground truths per (image, category)
        lab = gt_label.cpu()
        ci = torch.searchsorted(cats, lab).clamp_(max=nk - 1)
        known = cats[ci] == lab
        img = torch.repeat_interleave(torch.arange(ni), gper)
        cnt = torch.bincount((img * nk + ci)[known], minlength=ni * nk)
        max_g = int(cnt.max())
        if max_g > capi.BOX_AP_GT_MAX:
            w = int(cnt.argmax())
            raise BoxApCapError(f"stlpose {op}: the image at table position {w // nk} has {max_g} ground truths of category "
                                f"{int(cats[w % nk])}; the cap is {capi.BOX_AP_GT_MAX} (STL_BOX_AP_GT_MAX) per image and category", w // nk)
    slots = _match_slots(op, "boxes", boxes, scores, (("labels", labels), ("gt_boxes", gt_boxes), ("gt_area", gt_area),
                                                      ("gt_label", gt_label), ("gt_crowd", gt_crowd)), ni, nk, capi.BOX_AP_AREAS)
    dev = boxes.device
    b, s, l = boxes.contiguous(), scores.contiguous(), labels.contiguous()
    gb, ga, gl, gc = gt_boxes.contiguous(), gt_area.contiguous(), gt_label.contiguous(), gt_crowd.contiguous()
    do, go, ct = doff.to(dev), goff.to(dev), cats.to(dev)
    capi.call("stl_box_ap_match", b.data_ptr(), s.data_ptr(), l.data_ptr(), do.data_ptr(), n, max_n, gb.data_ptr(), ga.data_ptr(),
              gl.data_ptr(), gc.data_ptr(), go.data_ptr(), g, max_g, ni, ct.data_ptr(), nk, _doubles(iou_thrs), _doubles(area_ranges),
              *(t.data_ptr() for t in slots), _st())
    return slots


def _match_fake(det, scores, det_offsets, nk: int, num_areas: int):
    n = det.shape[0]
    return (det.new_empty(n, dtype=scores.dtype), det.new_empty(n, dtype=torch.int32), det.new_empty(n, dtype=torch.int32),
            det.new_empty(n, dtype=torch.int64), det.new_empty(n, dtype=torch.int64),
            det.new_empty(det_offsets.shape[0] - 1, nk, num_areas, dtype=torch.int32))


# slot_score, slot_cat (-1: the row is in no category's list), slot_rank, matched and ignored bits (bit t * 4 + a) per detection
# row, npig [I, K, 4]; the slot layout is stated at stl_box_ap_match in include/stlpose_hip.h
_define("box_ap_match(Tensor boxes, Tensor scores, Tensor labels, Tensor det_offsets, Tensor gt_boxes, Tensor gt_area, Tensor gt_label, "
        "Tensor gt_crowd, Tensor gt_offsets, Tensor categories, float[] iou_thrs, float[] area_ranges) "
        "-> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)", _box_ap_match,
        lambda b, s, l, do, gb, ga, gl, gc, go, cats, thrs, rng: _match_fake(b, s, do, cats.shape[0], capi.BOX_AP_AREAS))


def _box_ap_accumulate(matched, ignored, rank, order, cat_offsets, npig, num_thrs: int, max_dets, rec_thrs):
    op = "box_ap_accumulate"
    ns = _table(op, "matched", matched, torch.int64, "S")
    for name, t, dt in (("ignored", ignored, torch.int64), ("rank", rank, torch.int32), ("order", order, torch.int64)):
        if t.dim() != 1 or t.shape[0] != ns or t.dtype != dt:
            raise ValueError(f"stlpose {op}: {name} must be {dt} [S={ns}], got {t.dtype} {tuple(t.shape)}")
    if npig.dim() != 2 or npig.dtype != torch.int64 or npig.shape[1] < 1:
        raise ValueError(f"stlpose {op}: npig must be int64 [K, A], got {npig.dtype} {tuple(npig.shape)}")
    nk, na = npig.shape
    if cat_offsets.dim() != 1 or cat_offsets.shape[0] != nk + 1 or cat_offsets.dtype != torch.int64:
        raise ValueError(f"stlpose {op}: cat_offsets must be int64 [K + 1 = {nk + 1}], got {cat_offsets.dtype} {tuple(cat_offsets.shape)}")
    co = cat_offsets.cpu()
    if int(co[0]) < 0 or int(co[-1]) > ns or bool((co[1:] < co[:-1]).any()):
        raise ValueError(f"stlpose {op}: cat_offsets must rise within 0 .. S = {ns}")
    if num_thrs < 1 or num_thrs * na > 64:
        raise ValueError(f"stlpose {op}: {num_thrs} thresholds x {na} area ranges; a slot has 64 bits")
    if not 1 <= len(max_dets) <= capi.BOX_AP_MAXDETS_MAX:
        raise ValueError(f"stlpose {op}: {len(max_dets)} maxDets values; the cap is {capi.BOX_AP_MAXDETS_MAX} (STL_BOX_AP_MAXDETS_MAX)")
    nr = len(rec_thrs)
    if not 1 <= nr <= capi.BOX_AP_RECS_MAX:
        raise ValueError(f"stlpose {op}: {nr} recall points; the cap is {capi.BOX_AP_RECS_MAX} (STL_BOX_AP_RECS_MAX)")
    if rec_thrs[0] != 0.0 or not all(b > a for a, b in zip(rec_thrs[:-1], rec_thrs[1:])):
        raise ValueError(f"stlpose {op}: the recall points must rise from 0")
    if not matched.is_cuda:
        raise RuntimeError(f"stlpose {op}: matched must be on the GPU")
    dev = matched.device
    _same_device((("ignored", ignored), ("rank", rank), ("order", order), ("npig", npig)), dev)
    nm = len(max_dets)
    precision = torch.empty(num_thrs, nr, nk, na, nm, dtype=torch.float64, device=dev)
    recall = torch.empty(num_thrs, nk, na, nm, dtype=torch.float64, device=dev)
    m, i, r, o, p = matched.contiguous(), ignored.contiguous(), rank.contiguous(), order.contiguous(), npig.contiguous()
    c = co.to(dev)
    capi.call("stl_box_ap_accumulate", m.data_ptr(), i.data_ptr(), r.data_ptr(), o.data_ptr(), c.data_ptr(), p.data_ptr(), ns, nk,
              int(num_thrs), na, (capi.i32 * nm)(*[int(v) for v in max_dets]), nm, _doubles(rec_thrs), nr, precision.data_ptr(),
              recall.data_ptr(), _st())
    return precision, recall


# precision [T, R, K, A, M] and recall [T, K, A, M] (COCOeval.eval's), -1 where a (category, area range) has no ground truth to find
_define("box_ap_accumulate(Tensor matched, Tensor ignored, Tensor rank, Tensor order, Tensor cat_offsets, Tensor npig, int num_thrs, "
        "int[] max_dets, float[] rec_thrs) -> (Tensor, Tensor)", _box_ap_accumulate,
        lambda m, i, r, o, c, p, t, md, rt: (m.new_empty(t, len(rt), p.shape[0], p.shape[1], len(md), dtype=torch.float64),
                                             m.new_empty(t, p.shape[0], p.shape[1], len(md), dtype=torch.float64)))

# ------------------------------------------------------------------ pose scoring (csrc/keypoint_eval.hip, csrc/coco_match.inc; rescoring + OKS-NMS, COCOeval "keypoints")
# Every shape, dtype, device and cap the kernels rely on is checked here, before anything is launched.
def _pose_var(op: str, sigmas):
    """(2 sigma)^2 as the host code forms it, for exactly 17 joints."""
    import numpy as np
    if len(sigmas) != capi.POSE_JOINTS:
        raise ValueError(f"stlpose {op}: {len(sigmas)} sigmas; the device path is built for {capi.POSE_JOINTS} joints (use evaluate.oks_ap "
                         "on the host for another count)")
    return _doubles((np.asarray([float(v) for v in sigmas], np.float64) * 2) ** 2)


def _pose_rescore_nms(preds, boxes, offsets, in_vis_thr: float, oks_thr: float, sigmas, serial_sum: bool = False):
    op = "pose_rescore_nms"
    j = capi.POSE_JOINTS
    if preds.dim() != 3 or tuple(preds.shape[1:]) != (j, 3) or preds.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"stlpose {op}: preds must be float32 or float64 [P, {j}, 3], got {preds.dtype} {tuple(preds.shape)}")
    n = preds.shape[0]
    _table(op, "boxes", boxes, torch.float64, "P", n, tail=(6,), note=" (centre, scale, area, score)")
    var = _pose_var(op, sigmas)
    off, per = _ragged(op, "offsets", offsets, n)
    ni = per.numel()
    max_n = int(per.max()) if ni else 0
    if max_n > capi.POSE_NMS_MAX:
        raise BoxApCapError(f"stlpose {op}: the image at table position {int(per.argmax())} has {max_n} persons; the cap is "
                            f"{capi.POSE_NMS_MAX} (STL_POSE_NMS_MAX) per image", int(per.argmax()))
    if not preds.is_cuda:
        raise RuntimeError(f"stlpose {op}: preds must be on the GPU")
    dev = preds.device
    _same_device((("boxes", boxes),), dev)
    score = torch.empty(n, dtype=torch.float64, device=dev)
    keep = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.empty(ni, dtype=torch.int32, device=dev)
    p, b, o = preds.contiguous(), boxes.contiguous(), off.to(dev)
    capi.call("stl_pose_rescore_nms", p.data_ptr(), int(preds.dtype == torch.float64), int(bool(serial_sum)), b.data_ptr(), o.data_ptr(), ni, n, max_n,
              float(in_vis_thr), float(oks_thr), var, score.data_ptr(), keep.data_ptr(), count.data_ptr(), _st())
    return score, keep, count


# serial_sum: the mean confidence as one running sum (the reference's loop) instead of numpy's order (the host function's mean())
# score fp64 [P]; keep int32 [P]: per image segment the image-local rows of the kept persons in NMS order, then -1; count int32 [I]
_define("pose_rescore_nms(Tensor preds, Tensor boxes, Tensor offsets, float in_vis_thr, float oks_thr, float[] sigmas, "
        "bool serial_sum=False) "
        "-> (Tensor, Tensor, Tensor)", _pose_rescore_nms,
        lambda p, b, o, iv, ot, sg, ss=False: (p.new_empty(p.shape[0], dtype=torch.float64), p.new_empty(p.shape[0], dtype=torch.int32),
                                     p.new_empty(o.shape[0] - 1, dtype=torch.int32)))


def _oks_ap_match(kpts, scores, area, det_offsets, gt_kpts, gt_area, gt_bbox, gt_crowd, gt_numkp, gt_offsets, oks_thrs, area_ranges, sigmas):
    op = "oks_ap_match"
    j = capi.POSE_JOINTS
    n = _table(op, "kpts", kpts, torch.float64, "N", tail=(j, 3))
    for name, t in (("scores", scores), ("area", area)):
        if t is not None:
            _table(op, name, t, torch.float64, "N", n)
    g = _table(op, "gt_kpts", gt_kpts, torch.float64, "G", tail=(j, 3))
    _table(op, "gt_bbox", gt_bbox, torch.float64, "G", g, tail=(4,), note=" (x, y, w, h)")
    for name, t, dt in (("gt_area", gt_area, torch.float64), ("gt_crowd", gt_crowd, torch.uint8), ("gt_numkp", gt_numkp, torch.int32)):
        if t.dim() != 1 or t.shape[0] != g or t.dtype != dt:
            raise ValueError(f"stlpose {op}: {name} must be {dt} [G={g}], got {t.dtype} {tuple(t.shape)}")
    var = _pose_var(op, sigmas)
    doff, goff, gper, max_n = _match_images(op, n, g, det_offsets, gt_offsets, oks_thrs, area_ranges, "OKS", capi.OKS_AP_THRS,
                                            capi.OKS_AP_AREAS)
    ni = gper.numel()
    max_g = int(gper.max()) if ni else 0
    if max_g > capi.BOX_AP_GT_MAX:
        raise BoxApCapError(f"stlpose {op}: the image at table position {int(gper.argmax())} has {max_g} ground truths; the cap is "
                            f"{capi.BOX_AP_GT_MAX} (STL_BOX_AP_GT_MAX) per image", int(gper.argmax()))
    # slot_cat: the rows beyond the first STL_OKS_AP_DETS of an image stay out of the category
    slots = _match_slots(op, "kpts", kpts, scores, (("gt_kpts", gt_kpts), ("gt_area", gt_area), ("gt_bbox", gt_bbox), ("gt_crowd", gt_crowd),
                                                    ("gt_numkp", gt_numkp)) + ((("area", area),) if area is not None else ()), ni, 1,
                         capi.OKS_AP_AREAS)
    dev = kpts.device
    k, s, ar = kpts.contiguous(), scores.contiguous(), (area.contiguous() if area is not None else None)
    gk, ga, gb, gc, gn = gt_kpts.contiguous(), gt_area.contiguous(), gt_bbox.contiguous(), gt_crowd.contiguous(), gt_numkp.contiguous()
    do, go = doff.to(dev), goff.to(dev)
    capi.call("stl_oks_ap_match", k.data_ptr(), s.data_ptr(), ar.data_ptr() if ar is not None else None, do.data_ptr(), n, max_n,
              gk.data_ptr(), ga.data_ptr(), gb.data_ptr(), gc.data_ptr(), gn.data_ptr(), go.data_ptr(), g, max_g, ni, _doubles(oks_thrs),
              _doubles(area_ranges), var, *(t.data_ptr() for t in slots), _st())
    return slots


# the slots of box_ap_match for one category (0) and three area ranges (bit t * 3 + a), slot_score fp64; the layout is stated at
# stl_oks_ap_match in include/stlpose_hip.h.  area None: the area of the keypoints' bounding box
_define("oks_ap_match(Tensor kpts, Tensor scores, Tensor? area, Tensor det_offsets, Tensor gt_kpts, Tensor gt_area, Tensor gt_bbox, "
        "Tensor gt_crowd, Tensor gt_numkp, Tensor gt_offsets, float[] oks_thrs, float[] area_ranges, float[] sigmas) "
        "-> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)", _oks_ap_match,
        lambda k, s, a, do, gk, ga, gb, gc, gn, go, thrs, rng, sg: _match_fake(k, s, do, 1, capi.OKS_AP_AREAS))

# ------------------------------------------------------------------ the detector's device tail (csrc/detections.hip)
def _det_postprocess(reg, cls, anchors, images, threshold: float, xmax: float, ymax: float, iou_thr: float):
    op = "det_postprocess"
    if reg.dim() != 3 or reg.shape[2] != 4 or reg.dtype != torch.float32:
        raise ValueError(f"stlpose {op}: regression must be float32 [B, A, 4], got {reg.dtype} {tuple(reg.shape)}")
    b, a = reg.shape[:2]
    if cls.dim() != 3 or tuple(cls.shape[:2]) != (b, a) or cls.shape[2] < 1 or cls.dtype != torch.float32:
        raise ValueError(f"stlpose {op}: classification must be float32 [B={b}, A={a}, nc], got {cls.dtype} {tuple(cls.shape)}")
    if tuple(anchors.shape[-2:]) != (a, 4) or anchors.numel() != a * 4 or anchors.dtype != torch.float32:
        raise ValueError(f"stlpose {op}: anchors must be float32 [A={a}, 4], got {anchors.dtype} {tuple(anchors.shape)}")
    rec = capi.C.sizeof(capi.DetImage)
    if images is not None and (images.dtype != torch.uint8 or images.dim() != 1 or images.shape[0] != b * rec or not images.is_contiguous()):
        raise ValueError(f"stlpose {op}: images must be the uint8 [B={b} * {rec}] table of StlDetImage records, got {images.dtype} "
                         f"{tuple(images.shape)}")
    if not reg.is_cuda:
        raise RuntimeError(f"stlpose {op}: regression must be on the GPU")
    _same_device((("classification", cls), ("anchors", anchors), ("images", images)), reg.device)
    r, c, an = reg.contiguous(), cls.contiguous(), anchors.contiguous()
    k = capi.BOX_MAX
    boxes = torch.empty(b, k, 4, device=reg.device)
    scores = torch.empty(b, k, device=reg.device)
    labels = torch.empty(b, k, dtype=torch.int32, device=reg.device)
    count = torch.empty(b, dtype=torch.int32, device=reg.device)
    capi.call("stl_det_postprocess", r.data_ptr(), c.data_ptr(), an.data_ptr(), _ptr(images), b, a, c.shape[2], float(threshold),
              float(xmax), float(ymax), float(iou_thr), boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), count.data_ptr(), _st())
    return boxes, scores, labels, count


def _det_tables_fake(r):
    k = capi.BOX_MAX
    return (r.new_empty(r.shape[0], k, 4), r.new_empty(r.shape[0], k), r.new_empty(r.shape[0], k, dtype=torch.int32),
            r.new_empty(r.shape[0], dtype=torch.int32))


_define("det_postprocess(Tensor regression, Tensor classification, Tensor anchors, Tensor? images, float threshold, float xmax, "
        "float ymax, float iou_thr) -> (Tensor, Tensor, Tensor, Tensor)", _det_postprocess,
        lambda r, c, a, im, t, xm, ym, it: _det_tables_fake(r))


def _det_tables(op: str, boxes, scores, labels, count) -> int:
    """The [B, STL_BOX_MAX] tables of det_postprocess, contiguous; B."""
    k = capi.BOX_MAX
    b = _table(op, "count", count, torch.int32, "B")
    for name, t, dtype, tail in (("boxes", boxes, torch.float32, (k, 4)), ("scores", scores, torch.float32, (k,)),
                                 ("labels", labels, torch.int32, (k,))):
        _table(op, name, t, dtype, "B", b, tail)
        if not t.is_contiguous():
            raise ValueError(f"stlpose {op}: {name} must be contiguous")
    return b


def _det_append(boxes, scores, labels, count, image_ids, st_boxes, st_scores, st_labels, slots, slot0: int, cursor, parity: int,
                overflow) -> None:
    """One launch, no allocation and no sync: the batch's rows go behind cursor[parity], its slots to slots[slot0 ..]."""
    op = "det_append"
    b = _det_tables(op, boxes, scores, labels, count)
    if b > 1024:
        raise ValueError(f"stlpose {op}: {b} images in one batch (at most 1024)")
    _table(op, "image_ids", image_ids, torch.int64, "B", b)
    cap = _table(op, "st_boxes", st_boxes, torch.float64, "cap", None, (4,))
    _table(op, "st_scores", st_scores, torch.float32, "cap", cap)
    _table(op, "st_labels", st_labels, torch.int64, "cap", cap)
    ns = _table(op, "slots", slots, torch.int64, "slots", None, (3,))
    if slot0 < 0 or slot0 + b > ns:
        raise ValueError(f"stlpose {op}: slots {slot0} .. {slot0 + b - 1} of a table of {ns}")
    _table(op, "cursor", cursor, torch.int64, "2", 2)
    _table(op, "overflow", overflow, torch.int64, "1", 1)
    if parity not in (0, 1):
        raise ValueError(f"stlpose {op}: parity {parity} (0 or 1)")
    for name, t in (("count", count), ("image_ids", image_ids), ("st_boxes", st_boxes), ("st_scores", st_scores), ("st_labels", st_labels),
                    ("slots", slots), ("cursor", cursor), ("overflow", overflow)):
        if not t.is_contiguous():
            raise ValueError(f"stlpose {op}: {name} must be contiguous")
    if not boxes.is_cuda:
        raise RuntimeError(f"stlpose {op}: boxes must be on the GPU")
    _same_device((("scores", scores), ("labels", labels), ("count", count), ("image_ids", image_ids), ("st_boxes", st_boxes),
                  ("st_scores", st_scores), ("st_labels", st_labels), ("slots", slots), ("cursor", cursor), ("overflow", overflow)),
                 boxes.device)
    capi.call("stl_det_append", boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), count.data_ptr(), image_ids.data_ptr(), b,
              st_boxes.data_ptr(), st_scores.data_ptr(), st_labels.data_ptr(), cap, slots.data_ptr(), int(slot0), cursor.data_ptr(),
              int(parity), overflow.data_ptr(), _st())


_define("det_append(Tensor boxes, Tensor scores, Tensor labels, Tensor count, Tensor image_ids, Tensor(a!) st_boxes, Tensor(b!) st_scores, "
        "Tensor(c!) st_labels, Tensor(d!) slots, int slot0, Tensor(e!) cursor, int parity, Tensor(f!) overflow) -> ()", _det_append,
        lambda *a: None)

def _person_boxes(boxes, scores, labels, count, label: int, score_thr: float, iou_thr: float, aspect: float, crop_w: int, crop_h: int):
    """iou_thr < 0: the label / score filter alone (1 launch); otherwise NMS on the passing rows as well (3 launches)."""
    op = "person_boxes"
    b = _det_tables(op, boxes, scores, labels, count)
    if b > 1024:
        raise ValueError(f"stlpose {op}: {b} images in one batch (at most 1024)")
    if crop_w < 1 or crop_h < 1 or not aspect > 0:
        raise ValueError(f"stlpose {op}: crop {crop_w} x {crop_h}, aspect {aspect}")
    if not count.is_contiguous():
        raise ValueError(f"stlpose {op}: count must be contiguous")
    if not boxes.is_cuda:
        raise RuntimeError(f"stlpose {op}: boxes must be on the GPU")
    _same_device((("scores", scores), ("labels", labels), ("count", count)), boxes.device)
    n, dev = b * capi.BOX_MAX, boxes.device
    img = torch.empty(n, dtype=torch.int32, device=dev)
    out = [torch.empty(n, w, device=dev) if w else torch.empty(n, device=dev) for w in (4, 0, 2, 2, 6)]
    total = torch.empty(1, dtype=torch.int32, device=dev)
    nms = iou_thr >= 0
    work = torch.empty(max(1, int(capi.lib().stl_person_boxes_workspace(b, int(nms)))), dtype=torch.uint8, device=dev)
    capi.call("stl_person_boxes", boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), count.data_ptr(), b, int(label), float(score_thr),
              float(iou_thr), float(aspect), int(crop_w), int(crop_h), work.data_ptr(), img.data_ptr(), *[t.data_ptr() for t in out],
              total.data_ptr(), _st())
    return (img, *out, total)


def _person_boxes_fake(boxes, scores, labels, count, label, score_thr, iou_thr, aspect, crop_w, crop_h):
    n = boxes.shape[0] * capi.BOX_MAX
    return (boxes.new_empty(n, dtype=torch.int32), boxes.new_empty(n, 4), boxes.new_empty(n), boxes.new_empty(n, 2), boxes.new_empty(n, 2),
            boxes.new_empty(n, 6), boxes.new_empty(1, dtype=torch.int32))


_define("person_boxes(Tensor boxes, Tensor scores, Tensor labels, Tensor count, int label, float score_thr, float iou_thr, float aspect, "
        "int crop_w, int crop_h) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)", _person_boxes, _person_boxes_fake)

# ------------------------------------------------------------------ detector batches (csrc/det_batch.hip)
def _det_batch(canvas, src, src_off, src_hw, index, box_start, box_count, boxes, labels, draws, flip_enabled: bool, s1: int, gt_rows: int,
               want_stage1: bool):
    """One launch of stl_det_batch (include/stlpose_hip_det_batch.h) into canvas, fp32 [B, S, S, 3] (a plan's, or a new tensor); every
    shape, dtype and device the kernel relies on is checked here, nothing is read back."""
    op = "det_batch"
    if src.dim() != 1 or src.dtype != torch.uint8:
        raise ValueError(f"stlpose {op}: src must be the uint8 [bytes] image buffer, got {src.dtype} {tuple(src.shape)}")
    if not src.is_cuda:
        raise RuntimeError(f"stlpose {op}: the image buffer must be on the GPU")
    b = _table(op, "index", index, torch.int64, "B")
    if not 1 <= b <= capi.DET_BATCH_MAX:
        raise ValueError(f"stlpose {op}: {b} images in one batch (1 .. {capi.DET_BATCH_MAX})")
    _table(op, "src_off", src_off, torch.int64, "B", b)
    _table(op, "src_hw", src_hw, torch.int32, "B", b, (2,))
    n = _table(op, "box_start", box_start, torch.int64, "N")
    _table(op, "box_count", box_count, torch.int32, "N", n)
    m = _table(op, "boxes", boxes, torch.float32, "M", None, (4,))
    _table(op, "labels", labels, torch.int64, "M", m)
    tabs = [("src_off", src_off), ("src_hw", src_hw), ("index", index), ("box_start", box_start), ("box_count", box_count),
            ("boxes", boxes), ("labels", labels)]
    if draws is not None:
        _table(op, "draws", draws, torch.float64, "B", b)
        tabs.append(("draws", draws))
    if canvas.dim() != 4 or canvas.shape[1] != canvas.shape[2]:
        raise ValueError(f"stlpose {op}: canvas must be float32 [B={b}, S, S, 3], got {canvas.dtype} {tuple(canvas.shape)}")
    s = canvas.shape[1]
    _table(op, "canvas", canvas, torch.float32, "B", b, (s, s, 3))
    tabs.append(("canvas", canvas))
    if not (1 <= s1 <= capi.DET_BATCH_SIDE and 1 <= s <= capi.DET_BATCH_SIDE) or gt_rows < 0:
        raise ValueError(f"stlpose {op}: S1 {s1}, canvas {s} (1 .. {capi.DET_BATCH_SIDE}), gt_rows {gt_rows}")
    dev = src.device
    _same_device(tabs, dev)
    for name, t in [("src", src)] + tabs:
        if not t.is_contiguous():
            raise ValueError(f"stlpose {op}: {name} must be contiguous")
    stage1 = torch.empty(b if want_stage1 else 0, s1, s1, 3, dtype=torch.uint8, device=dev)
    gt = torch.empty(gt_rows, 5, dtype=torch.float32, device=dev)
    offsets = torch.empty(b + 1, dtype=torch.int32, device=dev)
    capi.call("stl_det_batch", src.data_ptr(), src.numel(), src_off.data_ptr(), src_hw.data_ptr(), index.data_ptr(), _ptr(box_start),
              _ptr(box_count), n, _ptr(boxes), _ptr(labels), m, _ptr(draws), int(bool(flip_enabled)), b, int(s1), int(s), canvas.data_ptr(),
              stage1.data_ptr() if want_stage1 else None, gt.data_ptr() if gt_rows else None, int(gt_rows), offsets.data_ptr(), _st())
    return stage1, gt, offsets


def _det_batch_fake(canvas, src, src_off, src_hw, index, box_start, box_count, boxes, labels, draws, flip_enabled, s1, gt_rows, want_stage1):
    b = index.shape[0]
    return (src.new_empty(b if want_stage1 else 0, s1, s1, 3), boxes.new_empty(gt_rows, 5), index.new_empty(b + 1, dtype=torch.int32))


# fills canvas; returns stage1 uint8 [B, s1, s1, 3] ([0, s1, s1, 3] unless asked for), gt fp32 [gt_rows, 5], offsets int32 [B + 1]
_define("det_batch(Tensor(a!) canvas, Tensor src, Tensor src_off, Tensor src_hw, Tensor index, Tensor box_start, Tensor box_count, "
        "Tensor boxes, Tensor labels, Tensor? draws, bool flip_enabled, int s1, int gt_rows, bool want_stage1) "
        "-> (Tensor, Tensor, Tensor)", _det_batch, _det_batch_fake)

OPS = ["person_mse", "heatmap_argmax", "final_preds", "flip_merge", "flip_merge_backward", "gaussian_targets", "affine_crop",
       "hrnet_forward", "hrnet_backward", "hrnet_backward_input", "pose_vectors", "pose_distances", "pose_topk", "pose_rank", "pose_rank_any",
       "box_select", "heatmap_resize_argmax", "det_decode", "det_nms", "det_loss", "box_ap_match", "box_ap_accumulate",
       "pose_rescore_nms", "oks_ap_match", "eval_tail", "eval_affine", "pose_augment", "det_postprocess", "det_append", "person_boxes", "det_batch"]
