"""The launch plans of the Python-listed models, built on the CPU (nothing is launched), and a signature of each list that
leaves out what differs from run to run: per entry its name and a CRC32 over its arguments, where a pointer counts only as null
or not, a descriptor as its fields (nested ones too, pointers again as null or not) and every other argument as its ``repr``.
What a signature cannot see, the offsets added to a base pointer, is listed in full next to it: the conv trunks' weight tables
(``*.wtab``) and the detector's pointwise pack offsets (``*.layout``).  The detector's training lists at every depth
(``DETECTOR_TRAIN``) also record which buffer each pointer names and the room behind it (``aliasing``).
tests/golden/launch/make_golden_launch.py records all of it, tests/test_launch_cpu.py compares."""
import ctypes as C
import zlib

import torch

CPU = torch.device("cpu")


def _fields(v):
    if isinstance(v, C.Structure):
        return [_fields(getattr(v, f[0])) if f[1] is not C.c_void_p else bool(getattr(v, f[0])) for f in v._fields_]
    if isinstance(v, C.Array):
        return [bool(x) if v._type_ is C.c_void_p else _fields(x) for x in v]
    return v.contents is not None if isinstance(v, C._Pointer) else v


def _arg(a, argtype):
    if argtype is C.c_void_p:
        return bool(a.value if isinstance(a, C.c_void_p) else a)
    if hasattr(argtype, "contents"):   # POINTER(descriptor): a byref
        return _fields(a._obj)
    return a


def _argtypes(e):
    """The argument types of a (name, args) or (fn, name, args) entry: the listed function's own (an entry point may live in any
    of the headers), or the main header's where the entry names no function."""
    from stlpose_amd import capi
    return e[0].argtypes if len(e) == 3 else capi.SIGNATURES[e[0]]


def signature(entries):
    """{"names": [...], "crc": [...]} of a list of (name, args) or (fn, name, args) entries."""
    names, crcs = [], []
    for e in entries:
        name, args = e[-2], e[-1]
        types = _argtypes(e)
        assert len(args) == len(types) - 1, name   # all but the stream
        names.append(name)
        crcs.append(zlib.crc32(repr([_arg(a, t) for a, t in zip(args, types)]).encode()))
    return {"names": names, "crc": crcs}


def wtab(tab, wk_elems, blocks, bias_off):
    """[every WPrep row as its field values, the number of ``wk`` elements, the block count of stl_weight_prep, ``bias_off``]."""
    return [[[getattr(e, f[0]) for f in e._fields_] for e in tab], wk_elems, blocks, list(bias_off)]


def vgg16():
    """A VGG16 perceptual trunk at 2x3x32x32."""
    from stlpose_amd import vgg
    m = vgg.VGGPerceptualLoss(resize=False)
    vgg.ready(m, CPU)
    t = m._plan(2, 32, 32, CPU)[0]
    return {"vgg16.ops": signature(t.ops), "vgg16.wtab": wtab(t.tab, t.wk.numel(), t.wblocks, m.bias_off)}


def vgg19():
    """A VGG19 style plan with the image gradient at 3 images of 32x32."""
    from stlpose_amd import vgg, vgg19_style
    m = vgg19_style.VGG19StyleLoss()
    vgg.ready(m, CPU)
    sp = vgg19_style.StylePlan(m, 3, 32, 32, CPU, 1, "batch", [0, 2], True)
    t = sp.trunk
    return {"vgg19.ops": signature(t.ops), "vgg19.bwd_ops": signature(sp.bwd_ops), "vgg19.wtab": wtab(t.tab, t.wk.numel(), t.wblocks, m.bias_off)}


def adain():
    """An AdaIN plan with its decoder at 1x32x32."""
    from stlpose_amd import adain
    m = adain.AdaINStylizer()
    m._pack(CPU)   # the host half of _ready: stl_weight_prep only fills ``wk``, no plan depends on it
    p = adain._Plan(m, 1, 32, 32, CPU, True)
    return {"adain.encode": signature(p.encode), "adain.decode": signature(p.decode),
            "adain.wtab": wtab(m.wtab, m.wk.numel(), m.wblocks, m.bias_off)}


def _d0_layout(m):
    """[[w, bias, Kp, Np] of every pointwise layer in packing order, [[w, offset, Kp, Np] of its transposed pack] (16-bit only)]."""
    L, pw = m._layout, []
    for lay in L["blocks"]:
        pw += [lay[k] for k in ("project", "expand") if k in lay]
    for lay in L["bifpn"]:
        pw += [v[1] if isinstance(v[1], tuple) else v for k, v in lay.items() if k != "weights"]
    for h in ("regressor", "classifier"):
        pw += [t for level in L[h]["pw"] for t in level] + [L[h]["hpw"]]
    tr = []
    if m.compute_dtype != "fp32":
        m._ensure_transposed()
        tr = [[w, *m._layoutT[w]] for w in sorted(m._layoutT)]
    return [[list(t) for t in pw], tr]


def d0(mode):
    """An EfficientDet-D0 plan at B = 1 with its counters and pointwise pack offsets and, where the heads train, its HeadTrain."""
    from stlpose_amd import detector_train, efficientdet
    m = efficientdet.EfficientDetBackbone(num_classes=2, compound_coef=0, compute_dtype=mode)
    p = m.plan(1, CPU)
    out = {f"d0.{mode}.calls": signature(p.calls), f"d0.{mode}.counts": [p.launches, p.flops, p.bytes, p.head_start]}
    if mode != "bf16":
        tr = detector_train.HeadTrain(m, p)
        pre = "d0.train" if mode == "fp32" else f"d0.{mode}.train"
        out[f"{pre}.fwd"], out[f"{pre}.bwd"] = signature(tr.fwd), signature(tr.bwd)
    out[f"d0.{mode}.layout"] = _d0_layout(m)
    return out


def _addresses(args, types):
    """Every address an entry passes, in argument order: its pointer arguments (a ``c_void_p`` object by its value) and the
    ``c_void_p`` fields of its descriptors, nested structures and arrays included; null is 0."""
    out = []

    def walk(v):
        if isinstance(v, C.Structure):
            for f in v._fields_:
                out.append(getattr(v, f[0]) or 0) if f[1] is C.c_void_p else walk(getattr(v, f[0]))
        elif isinstance(v, C.Array):
            for x in v:
                out.append(x or 0) if v._type_ is C.c_void_p else walk(x)

    for a, t in zip(args, types):
        if t is C.c_void_p:
            out.append((a.value if isinstance(a, C.c_void_p) else a) or 0)
        elif hasattr(t, "contents"):
            walk(a._obj)
    return out


def _tensors(v, out, seen):
    """The tensors that v holds: itself, or inside dicts, lists and tuples."""
    if isinstance(v, torch.Tensor):
        out.append(v)
    elif isinstance(v, (dict, list, tuple)) and id(v) not in seen:
        seen.add(id(v))
        for x in (v.values() if isinstance(v, dict) else v):
            _tensors(x, out, seen)


def _owners(keep, holders):
    """The memory that the tensors of ``keep`` and of the attributes of ``holders`` span, as sorted disjoint [start, end) byte
    ranges: a tensor inside a larger one (a view of the weight buffer, one level of a gradient table) counts as the larger one."""
    ts, seen = [], set()
    _tensors(keep, ts, seen)
    for h in holders:
        _tensors(list(vars(h).values()), ts, seen)
    spans = sorted({(t.data_ptr(), t.data_ptr() + t.element_size() * (1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))))
                    for t in ts if t.numel()}, key=lambda se: (se[0], -se[1]))
    out = []
    for s, e in spans:
        if out and e <= out[-1][1]:
            continue
        assert not out or s >= out[-1][1], "two tensors overlap without one holding the other"
        out.append((s, e))
    return out


def aliasing(plan, tr):
    """What ``signature`` cannot see of a detector training plan: which buffer each pointer names and how much room lies behind it.
    Walks ``plan.calls``, ``tr.fwd`` and ``tr.bwd`` in order; every distinct non-null address gets the ordinal of its first
    appearance (null: 0) and its room, the bytes from it to the end of the largest tensor that holds it, among the tensors of the
    lists' keep and of the attributes of the plan and of ``tr``.  An address that no tensor holds raises.  Returns
    {"fwd": [...], "bwd": [...]}: per entry one CRC32 over its (ordinal, room) pairs."""
    import bisect
    assert tr.fwd.keep is tr.bwd.keep
    spans = _owners([plan.calls.keep, tr.fwd.keep], [plan, tr])
    starts = [s for s, _ in spans]
    seen = {0: (0, 0)}   # address -> (ordinal, room)
    out = {}
    for key, entries in (("calls", plan.calls), ("fwd", tr.fwd), ("bwd", tr.bwd)):
        out[key] = []
        for i, e in enumerate(entries):
            pairs = []
            for a in _addresses(e[-1], _argtypes(e)):
                if a not in seen:
                    j = bisect.bisect_right(starts, a) - 1
                    if j < 0 or a >= spans[j][1]:
                        raise AssertionError(f"{key}[{i}] ({e[-2]}): address {a:#x} lies in no tensor of the plan, the lists or their keep")
                    seen[a] = (len(seen), spans[j][1] - a)
                pairs.append(seen[a])
            out[key].append(zlib.crc32(repr(pairs).encode()))
    del out["calls"]   # the trunk's launches take part in the numbering only
    return out


# key -> (compound coefficient, compute dtype, the setters called in order): the training depths of tests/golden/launch/detector_train.json
DETECTOR_TRAIN = {
    "d0.heads": (0, "fp32", ()),
    "d0.f16.heads": (0, "f16", ()),
    "d0.bifpn1": (0, "fp32", (("set_train_bifpn", 1),)),
    "d0.bifpn_all": (0, "fp32", (("set_train_bifpn", "all"),)),
    "d0.backbone1": (0, "fp32", (("set_train_bifpn", "all"), ("set_train_backbone", 1))),
    "d0.trunk6": (0, "fp32", (("set_train_bifpn", "all"), ("set_train_trunk", 6))),   # block 10 first: block 11 joins P4's gradient
    "d0.trunk_all": (0, "fp32", (("set_train_bifpn", "all"), ("set_train_trunk", "all"))),   # the block without an expand layer, the P3 join, the stem
    "d3.backbone2": (3, "fp32", (("set_train_bifpn", "all"), ("set_train_backbone", 2))),   # two heads-form blocks with a skip between them
    "d3.trunk_all": (3, "fp32", (("set_train_bifpn", "all"), ("set_train_trunk", "all"))),
}


def detector_train(key):
    """The training lists of one depth of DETECTOR_TRAIN at B = 1, built like ``d0``: {"fwd": ..., "bwd": ...}, each the list's
    ``signature`` with its ``aliasing`` CRCs as "alias"."""
    from stlpose_amd import detector_train as dt, efficientdet
    cc, mode, setup = DETECTOR_TRAIN[key]
    m = efficientdet.EfficientDetBackbone(num_classes=2, compound_coef=cc, compute_dtype=mode)
    for setter, k in setup:
        getattr(m, setter)(k)
    p = m.plan(1, CPU)
    tr = dt.HeadTrain(m, p)
    alias = aliasing(p, tr)
    return {which: dict(signature(getattr(tr, which)), alias=alias[which]) for which in ("fwd", "bwd")}


BUILDERS = {"vgg16": vgg16, "vgg19": vgg19, "adain": adain, "d0.fp32": lambda: d0("fp32"), "d0.bf16": lambda: d0("bf16"),
            "d0.f16": lambda: d0("f16")}
