"""The launch plans of the Python-listed models, built on the CPU (nothing is launched), and a signature of each list that
leaves out what differs from run to run: per entry its name and a CRC32 over its arguments, where a pointer counts only as null
or not, a descriptor as its fields (nested ones too, pointers again as null or not) and every other argument as its ``repr``.
tests/golden/launch/make_golden_launch.py records the signatures, tests/test_launch_cpu.py compares them."""
import ctypes as C
import zlib
from types import SimpleNamespace
from unittest import mock

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


def _adain_on_cpu(m):
    """AdaINStylizer._ready without its one device launch (stl_weight_prep, which fills ``wk``: no plan depends on it)."""
    from stlpose_amd import capi
    call = capi.call

    def host_only(name, *args):
        if name != "stl_weight_prep":
            call(name, *args)

    with mock.patch.object(capi, "call", host_only), mock.patch.object(torch.cuda, "current_stream", lambda: SimpleNamespace(cuda_stream=0)):
        m._ready(CPU)


def vgg16():
    """A VGG16 perceptual trunk at 2x3x32x32."""
    from stlpose_amd import vgg
    m = vgg.VGGPerceptualLoss(resize=False)
    vgg.ready(m, CPU)
    return {"vgg16.ops": signature(m._plan(2, 32, 32, CPU)[0].ops)}


def vgg19():
    """A VGG19 style plan with the image gradient at 3 images of 32x32."""
    from stlpose_amd import vgg, vgg19_style
    m = vgg19_style.VGG19StyleLoss()
    vgg.ready(m, CPU)
    sp = vgg19_style.StylePlan(m, 3, 32, 32, CPU, 1, "batch", [0, 2], True)
    return {"vgg19.ops": signature(sp.trunk.ops), "vgg19.bwd_ops": signature(sp.bwd_ops)}


def adain():
    """An AdaIN plan with its decoder at 1x32x32."""
    from stlpose_amd import adain
    m = adain.AdaINStylizer()
    _adain_on_cpu(m)
    p = adain._Plan(m, 1, 32, 32, CPU, True)
    return {"adain.encode": signature(p.encode), "adain.decode": signature(p.decode)}


def d0(mode):
    """An EfficientDet-D0 plan at B = 1 with its counters and, in fp32, its HeadTrain."""
    from stlpose_amd import detector_train, efficientdet
    m = efficientdet.EfficientDetBackbone(num_classes=2, compound_coef=0, compute_dtype=mode)
    p = m.plan(1, CPU)
    out = {f"d0.{mode}.calls": signature(p.calls), f"d0.{mode}.counts": [p.launches, p.flops, p.bytes, p.head_start]}
    if mode == "fp32":
        tr = detector_train.HeadTrain(m, p)
        out["d0.train.fwd"], out["d0.train.bwd"] = signature(tr.fwd), signature(tr.bwd)
    return out


BUILDERS = {"vgg16": vgg16, "vgg19": vgg19, "adain": adain, "d0.fp32": lambda: d0("fp32"), "d0.bf16": lambda: d0("bf16")}
