"""The launch plans of the Python-listed models, built on the CPU (nothing is launched), and a signature of each list that
leaves out what differs from run to run: per entry its name and a CRC32 over its arguments, where a pointer counts only as null
or not, a descriptor as its fields (nested ones too, pointers again as null or not) and every other argument as its ``repr``.
What a signature cannot see, the offsets added to a base pointer, is listed in full next to it: the conv trunks' weight tables
(``*.wtab``) and the detector's pointwise pack offsets (``*.layout``).
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


def signature(entries):
    """{"names": [...], "crc": [...]} of a list of (name, args) or (fn, name, args) entries."""
    from stlpose_amd import capi
    names, crcs = [], []
    for e in entries:
        name, args = e[-2], e[-1]
        types = capi.SIGNATURES[name]
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


BUILDERS = {"vgg16": vgg16, "vgg19": vgg19, "adain": adain, "d0.fp32": lambda: d0("fp32"), "d0.bf16": lambda: d0("bf16"),
            "d0.f16": lambda: d0("f16")}
