"""Static execution planner for the HRNet hot path on MI355X.

The network topology (``arch.walk``) is turned ONCE per (batch, resolution, dtype, mode) into two
flat lists of C-ABI kernel invocations with every device pointer resolved -- a forward program and
its hand-derived backward program -- which are then replayed eagerly or captured in a HIP graph.
No tracing compiler and no autograd tape at run time: the backward program is built here by a
reverse walk over the plan (``_build_backward``).

Data flow choices:
  * activations NHWC, dtype bf16 or fp32, fp32 accumulation, fp64 BatchNorm statistics;
  * a conv writes its RAW output plus per-channel sums; the BatchNorm (+ReLU) is applied by the
    consumer while it stages its input ("normalise on load"), so BN costs no HBM pass of its own;
  * residual adds / exchange sums are the only materialised activations (``fuse``);
  * backward mirrors it: the data-gradient conv masks with the ReLU and reduces the BatchNorm
    backward sums in its epilogue, and dgrad/wgrad apply the BatchNorm backward on load.
"""
from __future__ import annotations

import bisect
import ctypes as C
import math
import os
from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional, Tuple, Union

import torch

from . import capi
from .arch import Arch, Registry, registry, walk

EPS = 1e-5       # nn.BatchNorm2d default
MOMENTUM = 0.1   # reference HRnet.py:23 (fuse/transition BNs use the default, also 0.1)


def _esz(dtype: int) -> int:
    return capi.DTYPES[dtype & 0xff][0]


def choose_tile(B: int, Ho: int, Wo: int, stride: int, ks: int, esz: int, bn_cols: int = 64,
                maxpx: int = 128, maxhalo: int = 576) -> Tuple[int, int]:
    """Pick the output tile (TH virtual rows x TW columns, TH*TW <= 128) that wastes the fewest
    MFMA rows / halo loads while fitting LDS."""
    vrows = B * (Ho + 1)
    best, best_tile = -1.0, (1, min(Wo, maxpx))
    for tw in range(min(Wo, 4), min(Wo, maxpx) + 1):
        th = max(1, min(maxpx // tw, vrows))
        hr, hc = (th - 1) * stride + ks, (tw - 1) * stride + ks
        lds = hr * hc * 80 + bn_cols * (ks * ks * 64 + 16) + 8192
        if lds > 150 * 1024 or hr * hc > maxhalo:   # 576 halo pixels = 9 staging vectors per thread
            continue
        cols = math.ceil(Wo / tw) * tw
        rows = math.ceil(vrows / th) * th
        eff = (Wo / cols) * (B * Ho / rows) * (th * tw / float(maxpx))
        eff *= ((th * tw) / float(hr * hc) * stride * stride) ** 0.25  # mild halo penalty
        if eff > best:
            best, best_tile = eff, (th, tw)
    return best_tile


@dataclass
class BNInfo:
    idx: int
    C: int
    param_off: int   # gamma offset in master (beta at +C)
    buf_off: int     # running_mean offset in float buffers (running_var at +C)
    stats_off: int   # offset (doubles) in the stats / rstats arenas
    inv_count: float = 0.0


@dataclass
class ConvInfo:
    key: str
    Co: int
    Ci: int          # real input channels
    ks: int
    stride: int
    patch: bool
    master_off: int
    fwd_off: int = -1
    bwd_off: int = -1
    Cik: int = 0     # input channels as the kernel sees them (32 for the patch conv)


class Launch(NamedTuple):
    """One op of a program: a kernel launch with its descriptor, its stream and the dependency tokens it reads and writes
    (device pointers of tensors, ``C.addressof`` of descriptors whose results have no tensor of their own)."""
    name: str
    desc: C.Structure
    stream: int
    reads: list
    writes: list


class Bucket(NamedTuple):
    """A gradient bucket: a contiguous suffix [lo, hi) of the flat gradient buffer, closed as soon as every parameter in it
    has its slabs / BatchNorm reductions complete (backward finishes the last layers first).  Each bucket gets one ranged
    slab reduction + BN-gradient launch inside the program, so the step has no serial tail, and an event a data-parallel
    all-reduce can wait on: its last op, bwd_ops[op]."""
    lo: int
    hi: int
    op: int

    def __getitem__(self, key):   # b["lo"] as well as b.lo and b[0]: callers read buckets by field name
        return getattr(self, key) if isinstance(key, str) else tuple.__getitem__(self, key)


@dataclass
class Act:
    kind: str            # 'plain' | 'bn'
    t: torch.Tensor      # storage (flat uint8)
    B: int
    H: int
    W: int
    C: int
    bn: Optional[BNInfo] = None
    relu: bool = False
    needs_grad: bool = True
    consumers: int = 0
    producer: Optional[FuseNode] = None                      # plain: the sum that wrote it (None: the patch tensor)
    # ---- state of the backward builder (_build_backward)
    grads: List[torch.Tensor] = field(default_factory=list)  # plain: gradient contributions
    dt: Optional[torch.Tensor] = None                        # bn: grad wrt BN output (masked)
    bwd_seen: int = 0                                        # consumers already handled by the backward builder
    fused_du: Optional[torch.Tensor] = None                  # plain: masked gradient produced by a fused dgrad

    @property
    def ptr(self) -> int:
        return self.t.data_ptr()


# ---- the tape: forward nodes in forward order, walked in reverse by the backward builder
@dataclass
class ConvNode:
    x: Act
    y: Act
    conv: ConvInfo
    ks: int       # as launched (the patch conv is a 1x1 conv over 32-wide patches)
    stride: int
    stream: int


@dataclass
class FuseNode:
    terms: List[Tuple[Act, int, bool]]   # (input, upsample shift, ReLU of its BN applied on load)
    z: Act
    relu: bool
    op: Launch   # its forward launch

    @property
    def block_end(self) -> bool:
        """z = ReLU(BN(y) + skip), BN term first (same summation order as the sum kernel): a block end that its first
        consumer may form itself (STL_SRC_BNADD)."""
        return self.relu and [(a.kind, s) for a, s, _ in self.terms] == [("bn", 0), ("plain", 0)]

    @property
    def same_bn(self) -> List[Act]:
        """BN terms at the output's resolution: their BatchNorm-backward sums are reduced with the sum's gradient."""
        return [a for a, s, _ in self.terms if a.kind == "bn" and s == 0]


@dataclass
class HeadNode:
    x: Act
    key: str
    joints: int


@dataclass
class _OpenBucket:
    """The gradient bucket under construction (_bucket_close): the suffix [lo, hi) of the flat gradient buffer."""
    lo: int
    hi: int
    slab0: int = 0    # its first slab
    done: int = 0     # parameter elements of [lo, hi) whose gradient launches are planned
    reads: list = field(default_factory=list)   # tokens of the launches that write its slabs
    stream: int = 0                             # (unplaced) stream of its last weight gradient

    def add(self, off: int, size: int):   # the gradient launches of parameters [off, off + size) are planned
        self.done += size
        self.lo = min(self.lo, off)


class ParamStore:
    """Flat fp32 master / grad / buffer storage laid out in state_dict order."""

    def __init__(self, reg: Registry, device):
        self.reg = reg
        self.param_off: Dict[str, int] = {}
        off = 0
        for k, s in reg.params:
            self.param_off[k] = off
            off += int(math.prod(s)) if s else 1
        self.nparam = off
        self.buf_off: Dict[str, int] = {}
        self.nbt_idx: Dict[str, int] = {}
        off, n = 0, 0
        for k, s in reg.buffers:
            if k.endswith("num_batches_tracked"):
                self.nbt_idx[k] = n
                n += 1
            else:
                self.buf_off[k] = off
                off += int(math.prod(s))
        self.nbuf, self.nnbt = off, n
        self.device = device
        self.master = torch.zeros(self.nparam, dtype=torch.float32, device=device)
        self.grads = torch.zeros(self.nparam, dtype=torch.float32, device=device)
        self.bufs = torch.zeros(self.nbuf, dtype=torch.float32, device=device)
        self.nbt = torch.zeros(self.nnbt, dtype=torch.int64, device=device)


class Engine:
    """One plan: fixed batch/resolution/dtype/mode.

    input_grad: the backward program also produces dL/d(image) in ``self.dimg`` (fp32 NCHW): the stem's patch tensor gets a
    data gradient and ``stl_patch3x3_backward`` turns it into the image gradient.  A training plan keeps everything else as
    without the flag (same forward, same parameter gradients).  An eval plan (training=False) gets a data-gradient-only backward
    through the eval-mode network: BatchNorm backward with the running statistics (BNBWD sources read ``stats = NULL`` and an
    ``rstats`` arena that stays zero), no weight gradients, no slabs or buckets, nothing written to the running statistics or
    ``store.grads``; every reduction the backward kernels perform lands in ``self.sink``, which nothing reads.  Without the
    flag a plan is exactly what it was before the flag existed."""

    def __init__(self, arch: Arch, store: ParamStore, B: int, H: int, W: int, dtype: int, training: bool,
                 input_grad: bool = False):
        assert H % 32 == 0 and W % 32 == 0, "input H, W must be multiples of 32 (four stride-2 stages + 8x upsample)"
        self.arch, self.store, self.B, self.H, self.W = arch, store, B, H, W
        # dtype: capi.F32, capi.BF16 or capi.MIXED (= dt2(BF16, F16)).  self.dtype = element type of the GRADIENT tensors (and, in
        # the pure modes, of everything), self.fdtype = of the FORWARD tensors (raw conv outputs, sums, forward kernel-layout
        # weights): f16 in the mixed mode -- BatchNorm bounds their range, and 10 mantissa bits instead of 7 cut the distance
        # from the fp32 reference; gradients have no such bound and stay bf16.
        self.dtype_code = dtype
        self.math = capi.math_of(dtype)   # stl_conv.math of every forward conv launch (capi.F32X3: the fp32 plan, split-bf16 products)
        if self.math and (training or input_grad):
            raise NotImplementedError("stlpose_amd.Engine: " + capi.X3_NO_GRADIENTS)
        self.dtype, self.fdtype = dtype & 0xff, ((dtype >> 8) & 0xff) or (dtype & 0xff)
        self.ydtype = self.fdtype if self.fdtype != self.dtype else 0   # what the backward descriptors carry (0 = same)
        self.training = training
        self.input_grad = input_grad
        self.dev = store.device
        self.esz = _esz(dtype)
        self.tdtype = torch.float32 if self.dtype == capi.F32 else torch.bfloat16   # kernel-layout weights: just a byte container in the 16-bit modes
        self.lib = capi.lib()
        self.fwd_ops: List[Launch] = []
        self.bwd_ops: List[Launch] = []
        self.tape: List[Union[ConvNode, FuseNode, HeadNode]] = []
        self.convs: List[ConvInfo] = []
        self.bns: List[BNInfo] = []
        self._keep: List = []  # keep ctypes structs / tensors alive
        self._progs: Dict[str, C.c_void_p] = {}   # "fwd" / "bwd" -> native program
        self._fixups: Dict[str, List[Tuple]] = {}   # arena -> (descriptor, field, byte offset): see _fix
        self.act_bytes = 0
        self.generation = 0   # forward passes through this plan (hrnet._Fn stale-backward check)
        # static I/O
        self.img = torch.zeros(B, 3, H, W, dtype=torch.float32, device=self.dev)
        self.out: Optional[torch.Tensor] = None
        self.dout: Optional[torch.Tensor] = None
        self.dimg: Optional[torch.Tensor] = None   # input_grad: dL/d(img), fp32 NCHW
        # pass 1: count BN channels to size the statistics arenas
        nstat = bn_stat_elems(store.reg)
        self.stats = torch.zeros(max(nstat, 1), dtype=torch.float64, device=self.dev)
        self.rstats = torch.zeros(max(nstat, 1), dtype=torch.float64, device=self.dev) if training or input_grad else None
        # eval + input_grad: rstats above stays all-zero (eval-mode BatchNorm backward is v = gamma * rstd_running * dt), and the
        # reductions the backward kernels cannot skip (data-gradient epilogues, sums, upsamples) go here instead
        self.sink = torch.zeros(max(nstat, 1), dtype=torch.float64, device=self.dev) if input_grad and not training else None
        self.overflow = torch.full((1,), 2 ** 31 - 1, dtype=torch.int32, device=self.dev)   # range guard, see check_forward_range
        # ---- the planner's knobs (all of them; INTEGRATION.md lists what each is for and what was measured)
        env = os.environ.get
        self.nstreams = int(env("STLPOSE_STREAMS", "4"))          # HIP streams = hardware queues of the plan (4 compute pipes)
        # block-end sums z = ReLU(BN(y) + skip) formed by the consuming conv1 (STL_SRC_BNADD) for layers of at least this many
        # channels.  Bit-identical to the two-launch form and time-neutral on MI355X (round 3, all 69 eligible sums merged:
        # 15.50 vs 15.33-15.43 ms per step; C <= 32 / C <= 64 / C >= 64 / C >= 128 only: 15.53 / 15.51 / 15.45 / 15.36): the conv
        # re-forms the sum for every halo pixel and every output-channel block, which costs what the saved launch bought.
        self.merge_minc = int(env("STLPOSE_MERGE_MINC", "128"))
        self.bucket_mb = float(env("STLPOSE_BUCKET_MB", "64"))    # gradient bucket size (16 -> 32 MB: 16.79 -> 16.66 ms per step in round 2; 32 -> 64: 13.50 -> 13.42 in round 5)
        # block budget of a weight-gradient launch (a group shares it): 512 = two 8-wave blocks per CU, which hide each other's
        # tile latency (round 3, grouped launches: 128 / 256 / 512 / 768 blocks = 17.65 / 16.03 / 15.36 / 15.57 ms per step)
        # Weight-gradient blocks per launch.  Round 5: 256 / 128 instead of 512 / 256 -- ONE 8-wave block (128 VGPRs) per CU, resp.
        # 16-wave blocks (a whole CU's registers each) on HALF the CUs, so that the data-gradient chain always finds room: a
        # persistent weight-gradient block holds its CU for the whole launch (45 - 70 us), and beside 500 / 256 of them a data
        # gradient ran 2.3 - 4.5 x its own time while the weight gradient lost 3 - 17 % (tools/pair_probe.py,
        # profiles/r05_pair_*.txt); beside 256 / 128 it runs 1.45 - 1.6 x.  Step: 13.30 -> 13.12 ms.
        # (16-bit plans; the fp32 kernels' blocks are half as many waves per CU to begin with: 512 stays -- 48.6 vs 50.1 ms per step)
        self.wgrad_blocks = int(env("STLPOSE_WGRAD_BLOCKS", "256" if self.esz == 2 else "512"))
        self.wgrad_blocks_wide = int(env("STLPOSE_WGRAD_BLOCKS_WIDE", str(self.wgrad_blocks // 2)))
        # members per grouped launch (round 3 at 256 blocks: 1 / 2 / 4 / 8 = 15.87 / 15.64 / 16.03 / 17.51; 4 at 512 blocks: 15.36)
        self.wgrad_group = int(env("STLPOSE_WGRAD_GROUP", "4"))
        # the 64-channel 3x3 blocks (16 waves, one per CU: 256 per launch): eight layers per launch keep the split-K slabs at the
        # 32-channel kernel's size (a slab is the whole [Co][9][Ci] filter bank; 256 blocks over four layers would double them)
        self.wgrad_group_wide = int(env("STLPOSE_WGRAD_GROUP_WIDE", "8"))
        self._poison = env("STLPOSE_POISON", "0") != "0"          # debug: planned buffers start as NaNs (see _alloc)
        self._stream = 0
        self._side = None
        self._stats_used = 0
        self._wk_elems = 0
        walk(self, arch)
        self._check_stats_arena(nstat)
        self._finalize_weights()
        self._build_tables()
        if training or input_grad:
            self._build_backward()
        assert not self._fixups, "descriptor fields left pointing into arenas that were never allocated"

    def _check_stats_arena(self, nstat: int):
        """every layer's [NSHARD][2C] slice must lie inside the arenas: kernels add to them through raw pointers"""
        if self._stats_used != nstat:
            raise RuntimeError(f"engine: the plan uses {self._stats_used} statistics elements, the arenas hold {nstat}")

    # ------------------------------------------------------------------ allocation helpers
    def _alloc(self, nbytes: int) -> torch.Tensor:
        """Every planned buffer lives as long as the engine: kernels hold raw pointers, so a tensor
        that merely lost its last Python reference must never go back to the caching allocator."""
        self.act_bytes += nbytes
        t = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        if self._poison:   # debug (STLPOSE_POISON=1): every planned buffer starts as NaNs, so that a kernel which reads a location
            t.fill_(0xFF)  # nobody wrote -- and lets it reach a result -- shows up deterministically (0xFFFF / 0xFFFFFFFF = NaN)
        self._keep.append(t)
        return t

    def _act_tensor(self, B, H, W, C) -> torch.Tensor:
        return self._alloc(B * H * W * C * self.esz)

    def _fix(self, desc, attr: str, arena: str, off: int):
        """desc.attr = base of `arena` + off bytes, set by _resolve once the arena exists (the kernel-layout weights "wk",
        the split-K slabs "slab" and their table "slab_tab" are sized only when the plan is complete)."""
        self._fixups.setdefault(arena, []).append((desc, attr, off))

    def _resolve(self, arena: str, t: torch.Tensor):
        for desc, attr, off in self._fixups.pop(arena, []):
            setattr(desc, attr, t.data_ptr() + off)

    def _src(self, a: Act, relu: Optional[bool] = None) -> capi.Src:
        s = capi.Src()
        s.x = a.ptr
        if a.kind == "plain":
            s.mode = capi.SRC_PLAIN
            return s
        bn = a.bn
        s.mode = capi.SRC_BN
        s.relu = int(a.relu if relu is None else relu)
        st = self.store
        s.gamma = st.master.data_ptr() + 4 * bn.param_off
        s.beta = st.master.data_ptr() + 4 * (bn.param_off + bn.C)
        if self.training:
            s.stats = self.stats.data_ptr() + 8 * bn.stats_off
        else:
            s.rmean = st.bufs.data_ptr() + 4 * bn.buf_off
            s.rvar = st.bufs.data_ptr() + 4 * (bn.buf_off + bn.C)
        s.inv_count = bn.inv_count
        s.eps = EPS
        return s

    def _gsrc(self, y: Act) -> capi.Src:
        """Gradient of a conv's raw output, BatchNorm backward applied on load."""
        s = self._src(y)
        s.mode = capi.SRC_BNBWD
        s.x = y.dt.data_ptr()
        s.y = y.ptr
        s.rstats = self.rstats.data_ptr() + 8 * y.bn.stats_off
        return s

    # ------------------------------------------------------------------ builder protocol (arch.walk)
    def set_stream(self, s: int):
        self._stream = s % self.nstreams

    def stem_input(self) -> Act:
        B, H, W = self.B, self.H, self.W
        Ho, Wo = H // 2, W // 2
        t = self._act_tensor(B, Ho, Wo, 32)
        pd = capi.Patch()
        pd.dtype, pd.B, pd.H, pd.W, pd.stride = self.fdtype, B, H, W, 2
        pd.img, pd.out = self.img.data_ptr(), t.data_ptr()
        self.fwd_ops.append(Launch("stl_patch3x3", pd, 0, [], [t.data_ptr()]))
        self._patches = Act("plain", t, B, Ho, Wo, 32, needs_grad=self.input_grad)
        return self._patches

    def conv_bn(self, ck, bk, x: Act, cout, ks, stride, relu, patch=False) -> Act:
        st = self.store
        real_ci = 3 if patch else x.C
        ci = ConvInfo(ck, cout, real_ci, ks, stride, patch, st.param_off[ck + ".weight"], Cik=x.C)
        kks, kstride = (1, 1) if patch else (ks, stride)
        pad = 1 if kks == 3 else 0
        Ho, Wo = (x.H + 2 * pad - kks) // kstride + 1, (x.W + 2 * pad - kks) // kstride + 1
        # kernel-layout weights: forward [Co][taps][Cik]; data-gradient [Cik][taps][Co]
        ci.fwd_off = self._wk_elems
        self._wk_elems += cout * kks * kks * x.C
        if x.needs_grad and (self.training or self.input_grad):
            ci.bwd_off = self._wk_elems
            self._wk_elems += cout * kks * kks * x.C
        self.convs.append(ci)
        bn = BNInfo(len(self.bns), cout, st.param_off[bk + ".weight"], st.buf_off[bk + ".running_mean"],
                    self._stats_used, 1.0 / float(x.B * Ho * Wo))
        self._stats_used += capi.NSHARD * 2 * cout
        self.bns.append(bn)
        y = Act("bn", self._act_tensor(x.B, Ho, Wo, cout), x.B, Ho, Wo, cout, bn=bn, relu=relu)
        p = capi.Conv()
        p.dtype = self.fdtype
        p.B, p.Hi, p.Wi, p.Ci, p.Ho, p.Wo, p.Co = x.B, x.H, x.W, x.C, Ho, Wo, cout
        p.ks, p.stride, p.stuff = kks, kstride, 0
        p.math = self.math
        p.TH, p.TW, p.shape = 0, 0, -1
        capi.call("stl_conv_plan", C.byref(p))  # block shape + pixel tile, searched once
        reads, writes = [x.ptr], [y.ptr]
        pend = x.producer
        if (pend is not None and pend.block_end and x.consumers == 0 and kstride == 1 and kks in (1, 3)
                and pend.op.stream == self._stream and self.merge_minc <= x.C and capi.lib().stl_conv_bnadd_ok(C.byref(p)) == 1):
            # Residual block end z = ReLU(BN(y2) + skip) whose FIRST consumer is this convolution (the next unit's conv1: 3x3
            # in the branches, 1x1 in layer1 -- round 5): the sum is formed while the conv stages its tiles and written out once
            # (STL_SRC_BNADD + src_out) -- the stand-alone sum launch and one pass over the tensor go (HRnet.py:58-59, 88-100).
            (ybn, _, _), (skip, _, _) = pend.terms   # BN term first (see fuse)
            self.fwd_ops.remove(pend.op)
            p.src = self._src(ybn, relu=True)
            p.src.mode = capi.SRC_BNADD
            p.src.y = skip.ptr
            p.src_out = x.ptr
            reads, writes = [ybn.ptr, skip.ptr], [y.ptr, x.ptr]
        else:
            p.src = self._src(x)
        p.out = y.ptr
        if self.training:
            p.out_stats = self.stats.data_ptr() + 8 * bn.stats_off
        self._fix(p, "w", "wk", ci.fwd_off * self.esz)
        self.fwd_ops.append(Launch("stl_conv_forward", p, self._stream, reads, writes))
        x.consumers += 1
        self.tape.append(ConvNode(x, y, ci, kks, kstride, self._stream))
        return y

    def fuse(self, terms, relu) -> Act:
        terms = [(a, s, a.relu if a.kind == "bn" else False) for a, s in terms]
        if len(terms) == 1 and terms[0][2] and not relu:
            relu, terms = True, [(terms[0][0], terms[0][1], False)]  # relu(bn(y)) == fuse-level ReLU
        assert not any(tr for _, _, tr in terms), "ReLU inside a multi-term sum is not part of this network"
        base = [a for a, s, _ in terms if s == 0][0]
        B, H, W, Cc = base.B, base.H, base.W, base.C
        z = Act("plain", self._act_tensor(B, H, W, Cc), B, H, W, Cc)
        p = capi.Fuse()
        p.dtype, p.B, p.H, p.W, p.C, p.nterms, p.relu = self.fdtype, B, H, W, Cc, len(terms), int(relu)
        for i, (a, s, tr) in enumerate(terms):
            assert a.C == Cc and a.H << s == H and a.W << s == W, "fuse: term shape mismatch"
            p.t[i].src = self._src(a, relu=tr)
            p.t[i].shift = s
            a.consumers += 1
        p.out = z.ptr
        op = Launch("stl_fuse_forward", p, self._stream, [a.ptr for a, _, _ in terms], [z.ptr])
        z.producer = FuseNode(terms, z, relu, op)
        self.fwd_ops.append(op)
        self.tape.append(z.producer)
        return z

    def head(self, key, x: Act, joints) -> torch.Tensor:
        st = self.store
        self.out = torch.zeros(x.B, joints, x.H, x.W, dtype=torch.float32, device=self.dev)
        self.head_w = st.master.data_ptr() + 4 * st.param_off[key + ".weight"]
        self.head_b = st.master.data_ptr() + 4 * st.param_off[key + ".bias"]
        hd = capi.Head()
        hd.dtype, hd.B, hd.H, hd.W, hd.Ci, hd.J = self.fdtype, x.B, x.H, x.W, x.C, joints
        hd.x, hd.w, hd.bias, hd.out = x.ptr, self.head_w, self.head_b, self.out.data_ptr()
        self.fwd_ops.append(Launch("stl_head_forward", hd, 0, [x.ptr], [self.out.data_ptr()]))
        x.consumers += 1
        self.tape.append(HeadNode(x, key, joints))
        return self.out

    # ------------------------------------------------------------------ weights in kernel layout
    def _finalize_weights(self):
        self.wk = torch.zeros(max(self._wk_elems, 1), dtype=self.tdtype, device=self.dev)
        self._resolve("wk", self.wk)
        tab, blk = [], 0
        for c in self.convs:
            tab.append(capi.WPrep(c.master_off, c.fwd_off, c.bwd_off, c.Co, c.Ci, c.ks, c.Cik, int(c.patch), blk))
            blk += math.ceil(c.Co * c.Ci * c.ks * c.ks / 1024)
        self._wprep_blocks = blk
        self._wprep_tab = _to_device((capi.WPrep * len(tab))(*tab), self.dev)
        self._wprep_n = len(self.convs)

    def _active_of(self, key: str) -> int:
        """Branch chains in flight around the layer `key` (its stage's branch count)."""
        if key.startswith("stage"):
            return int(key[5])
        if key.startswith("transition") and key[10] in "23":
            return int(key[10])
        return 1 if not key.startswith("final") else self.nstreams

    # ------------------------------------------------------------------ backward program
    def _new_grad(self, a: Act) -> torch.Tensor:
        return self._act_tensor(a.B, a.H, a.W, a.C)

    def _red(self, bn: BNInfo) -> int:
        """Where a BatchNorm's backward reductions go: rstats, or the sink of an eval plan."""
        return self._red_arena.data_ptr() + 8 * bn.stats_off

    def _build_backward(self):
        self.slabs: List[capi.Slab] = []   # the slab reduction's table, one entry per weight-gradient partial sum
        self._slab_elems = 0               # fp32 elements of the slab arena
        self._slab_blocks = 0              # blocks of the slab reduction
        self.dout = torch.zeros_like(self.out)
        self._red_arena = self.rstats if self.training else self.sink   # eval plans (input_grad) compute data gradients only
        self._wg_pending: Dict[Tuple, List[Launch]] = {}   # grouped weight gradients waiting for their group to fill
        self.sched_estimate_us = [0.0] * self.nstreams     # per stream: estimated time of its launches so far (_emit)
        self._active = self.nstreams   # branch streams busy with the data-gradient chain around the node being walked
        self.buckets: List[Bucket] = []
        self._bucket = _OpenBucket(self.store.nparam, self.store.nparam)
        node_backward = {HeadNode: self._head_backward, FuseNode: self._fuse_backward, ConvNode: self._conv_backward}
        for node in reversed(self.tape):
            if isinstance(node, ConvNode):
                self._active = min(self.nstreams, self._active_of(node.conv.key))
            if self.training:
                self._bucket_close()   # after the previous node's ops: closes a bucket when a complete suffix is large enough
            node_backward[type(node)](node)
        if self.training:
            self._bucket_close(force=True)
            assert self._bucket.done == 0 and self._bucket.hi == 0, "gradient buckets do not cover the parameter buffer"
        if self.input_grad:
            self._emit_patch_backward()
        self.slab_arena = torch.zeros(max(self._slab_elems, 1), dtype=torch.float32, device=self.dev)
        self._resolve("slab", self.slab_arena)
        if self.training:
            self._slab_tab = _to_device((capi.Slab * len(self.slabs))(*self.slabs), self.dev)
            self._resolve("slab_tab", self._slab_tab)

    def _head_backward(self, n: HeadNode):
        x, J, st = n.x, n.joints, self.store
        x.bwd_seen += 1
        nblk = max(1, min(256, math.ceil(x.B * x.H * x.W / 256)))   # <= one 256-pixel chunk per block
        dx = self._new_grad(x)
        nel = J * x.C + J
        hb = capi.HeadBwd()
        hb.dtype, hb.B, hb.H, hb.W, hb.Ci, hb.J, hb.nblk = capi.dt2(self.dtype, self.fdtype), x.B, x.H, x.W, x.C, J, nblk
        hb.x, hb.w, hb.dout, hb.dx = x.ptr, self.head_w, self.dout.data_ptr(), dx.data_ptr()
        part_off = self._slab_alloc(hb, nblk * nel)
        self._emit("stl_head_backward", hb, 0, [self.dout.data_ptr(), x.ptr], [dx.data_ptr(), C.addressof(hb)])
        x.grads.append(dx)
        if not self.training:   # the kernel still writes its weight-gradient partials: into the slab arena, unreduced
            return
        w_off, b_off = st.param_off[n.key + ".weight"], st.param_off[n.key + ".bias"]
        self._bucket.reads.append(C.addressof(hb))
        self._bucket.add(w_off, J * x.C + J)   # the bias follows the weight
        self._add_slab(part_off, w_off, nblk, J, x.C, 1, x.C, 0, stride=nel)
        self._add_slab(part_off + J * x.C, b_off, nblk, J, 1, 1, 1, 0, stride=nel)

    def _fuse_backward(self, n: FuseNode):
        z = n.z
        for a, _s, _ in n.terms:
            a.bwd_seen += 1
        if z.fused_du is not None:
            # the ReLU mask, the BatchNorm reductions and the sum of contributions were done in the
            # epilogue of the data gradient that produced the last contribution (mask_z)
            assert not z.grads
            z.grads.append(z.fused_du)
        grads, same_bn = z.grads, n.same_bn
        assert 1 <= len(grads) <= 4, f"fuse output has {len(grads)} gradient contributions"
        if (len(grads) == 1 and not n.relu and not same_bn) or z.fused_du is not None:
            du = grads[0]   # nothing left to do: the gradient passes through
        else:
            du = self._new_grad(z)
            p = capi.FuseBwd()
            p.dtype, p.B, p.H, p.W, p.C = self.dtype, z.B, z.H, z.W, z.C
            p.ydtype = self.ydtype
            p.ngrads, p.relu = len(grads), int(n.relu)
            for i, gt in enumerate(grads):
                p.dz[i] = gt.data_ptr()
            p.z = z.ptr
            p.nbn = len(same_bn)
            for i, a in enumerate(same_bn):
                p.bn[i] = self._src(a)
                p.rstats[i] = self._red(a.bn)
            p.du = du.data_ptr()
            self._emit("stl_fuse_backward", p, n.op.stream, [gt.data_ptr() for gt in grads], [du.data_ptr()])
        for a, s, _ in n.terms:
            if a.kind == "plain":
                assert s == 0, "upsampled plain terms do not occur in this network"
                if a.needs_grad:
                    a.grads.append(du)
            elif s == 0:
                a.dt = du
            else:   # the adjoint of the nearest upsample, with the BatchNorm-backward sums of the term
                u = capi.UpBwd()
                u.dtype, u.B, u.H, u.W, u.C, u.shift = self.dtype, a.B, a.H, a.W, a.C, s
                u.ydtype = self.ydtype
                u.du = du.data_ptr()
                a.dt = self._new_grad(a)
                u.dt = a.dt.data_ptr()
                u.bn = self._src(a)
                u.rstats = self._red(a.bn)
                self._emit("stl_upsample_backward", u, n.op.stream, [du.data_ptr()], [a.dt.data_ptr()])

    def _conv_backward(self, n: ConvNode):
        """Weight gradient (training plans) and data gradient of one convolution."""
        x, y, ci = n.x, n.y, n.conv
        x.bwd_seen += 1
        assert y.consumers == 1 and y.dt is not None, f"{ci.key}: BN activation must have exactly one consumer"
        g = self._gsrc(y)
        if self.training:
            self._emit_wgrad(n, g)
            self._bucket.add(ci.master_off, ci.Co * ci.Ci * ci.ks * ci.ks)
            self._bucket.add(y.bn.param_off, 2 * y.bn.C)   # gamma, beta of the BatchNorm behind this conv
        if not x.needs_grad:
            return
        d = capi.Conv()
        d.dtype, d.ydtype = self.dtype, self.ydtype
        d.B, d.Hi, d.Wi, d.Ci = y.B, y.H, y.W, y.C
        d.Ho, d.Wo, d.Co = x.H, x.W, x.C
        d.ks, d.stride, d.stuff = n.ks, 1, int(n.stride == 2)
        d.TH, d.TW, d.shape = 0, 0, -1
        d.src = g   # (before the plan: data gradients get a block shape of their own)
        capi.call("stl_conv_plan", C.byref(d))
        d.w = self.wk.data_ptr() + ci.bwd_off * self.esz
        reads = [y.dt.data_ptr()]
        out = self._new_grad(x)
        if x.kind == "bn":
            assert x.dt is None
            x.dt = out
            d.mask_y = x.ptr
            d.mask_bn = self._src(x)
            d.red = self._red(x.bn)
        else:
            if x.grads:
                ad = x.grads.pop()
                d.addend = ad.data_ptr()
                reads.append(ad.data_ptr())
            # Residual block end z = ReLU(BN(y) + skip): when this data gradient is the LAST
            # contribution to dz, its epilogue also applies the ReLU mask and reduces the
            # BatchNorm-backward sums, so no separate pass over dz / z / y is needed.
            F = x.producer
            if F is not None and F.relu and len(F.same_bn) == 1 and not x.grads and x.bwd_seen == x.consumers:
                ybn = F.same_bn[0]
                d.mask_z = x.ptr
                d.mask_y = ybn.ptr
                d.mask_bn = self._src(ybn, relu=False)
                d.red = self._red(ybn.bn)
                reads += [x.ptr, ybn.ptr]
                x.fused_du = out
            else:
                x.grads.append(out)
        d.out = out.data_ptr()
        self._emit("stl_conv_forward", d, n.stream, reads, [out.data_ptr()])

    def _emit_patch_backward(self):
        """Image gradient: the adjoint of the stem's patch gather (stl_patch3x3_backward) over the patch tensor's data gradient,
        which the stem conv's data-gradient launch (a 1x1 conv onto 32-wide patches, weights [kk][Co]) has just written."""
        x = self._patches
        assert len(x.grads) == 1 and x.bwd_seen == x.consumers == 1, "patch tensor: expected one data-gradient contribution"
        self.dimg = torch.zeros(self.B, 3, self.H, self.W, dtype=torch.float32, device=self.dev)
        pb = capi.PatchBwd()
        pb.dtype, pb.B, pb.H, pb.W, pb.stride = self.dtype, self.B, self.H, self.W, 2
        pb.dpatch, pb.dimg = x.grads[0].data_ptr(), self.dimg.data_ptr()
        self._emit("stl_patch3x3_backward", pb, 0, [pb.dpatch], [pb.dimg])

    def _slab_alloc(self, desc, nelem: int) -> int:
        """Room for `nelem` weight-gradient partial sums of `desc` in the slab arena: their offset (fp32 elements), where
        desc.partial points once the arena exists."""
        off = self._slab_elems
        self._fix(desc, "partial", "slab", 4 * off)
        self._slab_elems += (nelem + 3) // 4 * 4   # keep every entry 16-byte aligned
        return off

    def _add_slab(self, part_off, grad_off, nsplit, Co, Ci, ks, Cip, patch, stride=0):
        self.slabs.append(capi.Slab(part_off, grad_off, nsplit, Co, Ci, ks, Cip, patch, self._slab_blocks, stride))
        self._slab_blocks += math.ceil(Co * Ci * ks * ks / 1024)

    def _bucket_close(self, force: bool = False):
        """Emit the open bucket's slab reduction and BatchNorm gradients, every field final, if the bucket is complete and
        large enough (or forced); the next bucket opens below it."""
        bk, st = self._bucket, self.store
        complete = bk.done == bk.hi - bk.lo          # suffix [lo, hi) fully covered
        # The serial tail of backward (layer1 + stem: one branch, 113 MB tensors) finishes last.  Close a bucket
        # where it begins, whatever its size, so that the final slab reduction (the only work left after the last
        # weight gradient, in front of the optimiser) covers just the stem / layer1 slabs instead of every layer
        # since the last 16 MB boundary.
        force = force or (complete and bk.lo in {st.param_off.get(k) for k in ("transition1.0.0.weight", "layer1.1.conv1.weight")})
        if not complete or bk.done == 0 or (bk.done < int(self.bucket_mb * (1 << 20) / 4) and not force):
            return
        for key in list(self._wg_pending):            # the bucket's slab reduction reads every member's slabs
            self._flush_wgrad_group(key)
        grads = st.grads.data_ptr()
        blk0 = self.slabs[bk.slab0].blk0   # (done > 0: the bucket has slabs)
        rr = capi.ReduceRange(grads=grads, n=len(self.slabs) - bk.slab0, blk_base=blk0, nblocks=self._slab_blocks - blk0)
        self._fix(rr, "partials", "slab", 0)
        self._fix(rr, "tab", "slab_tab", bk.slab0 * C.sizeof(capi.Slab))
        i0, i1 = bisect.bisect_left(self._bn_offs, bk.lo), bisect.bisect_left(self._bn_offs, bk.hi)
        br = capi.BNRange(rstats=self.rstats.data_ptr(), grads=grads, tab=self._bn_tab.data_ptr() + i0 * C.sizeof(capi.BNRec),
                          n=i1 - i0)
        self._emit("stl_reduce_slabs_range", rr, bk.stream, bk.reads, [C.addressof(rr)])
        self._emit("stl_bn_grads_range", br, bk.stream, [C.addressof(rr)], [C.addressof(br)])
        self.buckets.append(Bucket(bk.lo, bk.hi, len(self.bwd_ops) - 1))
        bk.hi, bk.done, bk.slab0, bk.reads = bk.lo, 0, len(self.slabs), []

    def _op_cost_us(self, name: str, d) -> float:
        """Rough duration of a backward launch for the list scheduler: a fixed launch + latency-chain part plus its
        bytes at ~2 TB/s (what these launches achieve)."""
        esz = self.esz
        if name == "stl_conv_forward":
            src = d.B * d.Hi * d.Wi * d.Ci * (2 if d.src.mode == capi.SRC_BNBWD else 1)
            out = d.B * d.Ho * d.Wo * d.Co * (1 + bool(d.mask_y) + bool(d.addend) + bool(d.mask_z))
            return 12.0 + (src + out) * esz / 2.0e6
        if name == "stl_conv_wgrad":
            by = (d.B * d.Hi * d.Wi * d.Ci + d.B * d.Ho * d.Wo * d.Co * (2 if d.g.mode == capi.SRC_BNBWD else 1)) * esz
            return 16.0 + (by + 2.0 * d.nsplit * d.Co * d.Ci * d.ks * d.ks * 4) / 2.0e6
        if name == "stl_conv_wgrad_group":
            m = d.members[0]
            by = (m.B * m.Hi * m.Wi * m.Ci + m.B * m.Ho * m.Wo * m.Co * (2 if m.g.mode == capi.SRC_BNBWD else 1)) * esz
            return 16.0 + d.n * (by + 2.0 * m.nsplit * m.Co * m.Ci * m.ks * m.ks * 4) / 2.0e6
        if name == "stl_fuse_backward":
            return 8.0 + d.B * d.H * d.W * d.C * (d.ngrads + 2 + d.nbn) * esz / 3.0e6
        if name == "stl_upsample_backward":
            return 8.0 + d.B * d.H * d.W * d.C * ((1 << (2 * d.shift)) + 2) * esz / 3.0e6
        if name == "stl_head_backward":
            return 80.0
        if name == "stl_reduce_slabs_range":
            return 20.0 + 80.0 * d.nblocks / 1100.0
        return 5.0

    def _emit(self, name: str, desc, stream: int, reads: list, writes: list):
        """Append a backward launch; an off-chain one (weight gradient, slab reduction, BatchNorm gradients) is placed here,
        statically, onto the branch streams -- one hardware queue each.  (With extra weight-gradient streams two
        streams share a queue and every switch between them costs ~6 us: 475 such gaps per step in
        profiles/r02_trace_default_summary.txt; on its own branch stream a weight gradient delays the
        data-gradient chain.)  Where the network has fewer branches than streams -- stage 3, stage 2, and the
        single-branch tail (layer1, stem), 40 % of backward -- the idle queues take the off-chain work: each such
        launch goes to the least-loaded stream among the idle ones and its own, by accumulated estimated time.
        In the tail only TWO idle queues are used: its launches stream 113 MB tensors at 3-4 TB/s each, and three
        weight gradients beside the data-gradient chain slow every one of them down by more than the overlap
        buys (round 2, tail queues 3 / 2 / 1 / 0: 16.98 / 16.86 / 16.82 / 17.33 ms per step; round 3 with ungrouped
        tail launches 3 / 2 / 1: 14.87 / 14.72 / 14.82)."""
        acc = self.sched_estimate_us
        if name in ("stl_conv_wgrad", "stl_conv_wgrad_group", "stl_reduce_slabs_range", "stl_bn_grads_range"):
            own = stream % self.nstreams
            cands = list(range(self._active, self.nstreams)) + [own]
            if self._active == 1:   # the single-branch tail: TWO of its three idle queues (see above)
                cands = list(range(1, min(3, self.nstreams))) + [own]
            stream = min(cands, key=lambda s_: (acc[s_], s_ != own))
        acc[stream] += self._op_cost_us(name, desc)
        self.bwd_ops.append(Launch(name, desc, stream, reads, writes))

    def _emit_wgrad(self, n: ConvNode, g: capi.Src):
        """Weight-gradient launch of one convolution (split-K slabs): off the critical path (only the data-gradient chain
        is on it); _emit places it on an idle queue where there is one."""
        x, y, ci, kks, kstride = n.x, n.y, n.conv, n.ks, n.stride
        wg = capi.Wgrad()
        wg.dtype, wg.ydtype = self.dtype, self.ydtype
        wg.B, wg.Hi, wg.Wi, wg.Ci, wg.Ho, wg.Wo, wg.Co = x.B, x.H, x.W, x.C, y.H, y.W, y.C
        wg.ks, wg.stride = kks, kstride
        ctile = capi.lib().stl_wgrad_chunk(C.byref(wg))   # 32, or 64: the 1x1 layers' wide kernel and the 16-wave 3x3 blocks (C >= 64)
        wide3 = ctile == 64 and kks == 3   # 64 x 64 channels per 1024-thread block: ONE block per CU, up to eight layers per launch
        wg.TH, wg.TW = choose_tile(x.B, y.H, y.W, kstride, kks, self.esz, bn_cols=32, maxhalo=(256 if wide3 else 192) if ctile == 64 else 576)   # (256 halo pixels: two staging vectors per thread of the 16-wave block)
        npt = math.ceil(x.B * (y.H + 1) / wg.TH) * math.ceil(y.W / wg.TW)
        chunks = math.ceil(y.C / ctile) * math.ceil(x.C / ctile)
        budget = self.wgrad_blocks_wide if wide3 else self.wgrad_blocks
        # The single-branch tail of backward (layer1, stem, transition1) is one serial data-gradient chain beside three idle
        # queues: a group there fills only when the chain has walked through ALL its members (every layer1 group completes
        # at the first block, i.e. at the very end of the step), so grouped weight gradients pile up behind the chain:
        # tail launches are not grouped (round 3, groups of 4 / 2 / 1: 15.02 / 14.81 / 14.82 ms per step).
        tail = self._active_of(ci.key) == 1
        gmax = self.wgrad_group_wide if wide3 else self.wgrad_group
        gsize = 1 if tail else max(1, min(gmax, capi.WGRAD_GROUP_MAX, max(1, budget // chunks)))
        # Grouped launches (stl_conv_wgrad_group): weight gradients of one shape -- the 3x3 convolutions of a branch --
        # wait until `gsize` of them are ready and go out as ONE launch that shares the block budget: the four hardware
        # queues carry one off-chain launch instead of gsize (in stages 3 / 4 every queue is busy with a data-gradient
        # chain and each stand-alone weight gradient costs its chain a full launch latency, whatever its size), every
        # block walks gsize times as many pixel tiles, and gsize times fewer split-K slabs are written and reduced.
        bg = budget // gsize
        top = max(1, min(npt, bg // chunks if chunks <= bg else 1))
        wg.nsplit = min(range(1, top + 1), key=lambda ns: (math.ceil(npt / ns) + 0.004 * ns * chunks / 8, ns))
        wg.h = self._src(x)
        wg.g = g
        part_off = self._slab_alloc(wg, wg.nsplit * y.C * kks * kks * x.C)
        self._add_slab(part_off, ci.master_off, wg.nsplit, ci.Co, ci.Ci, ci.ks, ci.Cik, int(ci.patch))
        self._bucket.reads.append(C.addressof(wg))
        self._bucket.stream = n.stream
        key = (x.C, y.C, kks, kstride, x.H, x.W, wg.TH, wg.TW, wg.nsplit, int(g.mode), gsize)
        pend = self._wg_pending.setdefault(key, [])
        pend.append(Launch("stl_conv_wgrad", wg, n.stream, [y.dt.data_ptr(), x.ptr], [C.addressof(wg)]))
        if len(pend) >= gsize:
            self._flush_wgrad_group(key)

    def _flush_wgrad_group(self, key):
        pend = self._wg_pending.pop(key)
        if len(pend) == 1:
            self._emit(*pend[0])
            return
        members = [op.desc for op in pend]
        grp = capi.WgradGroup()
        grp.n = len(members)
        for i, wg in enumerate(members):
            grp.p[i] = C.pointer(wg)
        grp.members = members   # python-side view (bench, tools); keeps the members alive
        self._emit("stl_conv_wgrad_group", grp, pend[-1].stream, [r for op in pend for r in op.reads],
                   [w for op in pend for w in op.writes])

    def _build_tables(self):
        tab = [capi.BNRec(b.stats_off, b.param_off, b.buf_off, b.C, b.inv_count) for b in self.bns]
        self._bn_tab = _to_device((capi.BNRec * len(tab))(*tab), self.dev)
        # num_batches_tracked entries are in registry (state_dict) order == self.bns order
        assert len(self.bns) == self.store.nnbt
        self._bn_offs = [b.param_off for b in self.bns]   # ascending: a bucket's BatchNorm range is found by bisection
        assert self._bn_offs == sorted(self._bn_offs)

    # ------------------------------------------------------------------ execution
    def _schedule(self, ops: List[Launch], recorded) -> Tuple[List[List[int]], set]:
        """Cross-stream RAW dependencies: op index -> indices it must wait for / whether it records (a waited-for op, or
        one of `recorded`).  A wait is dropped when the consumer's stream already knows the producer to be complete --
        directly (an earlier wait on the same or a later op of that stream) or transitively (vector clocks: 41 of 183
        waits of the W32 backward)."""
        last, waits, need = {}, [], set(recorded)
        ns = max(o.stream for o in ops) + 1 if ops else 1
        clock = [[-1] * ns for _ in range(ns)]   # clock[s][t]: latest op of stream t known complete at this point of stream s
        snap = {}
        for i, op in enumerate(ops):
            s = op.stream
            w = set()
            for r in op.reads:
                j = last.get(r)
                if j is not None and ops[j].stream != s:
                    w.add(j)
            latest = {}
            for j in w:                      # streams are in-order: the latest producer per stream covers the others
                latest[ops[j].stream] = max(latest.get(ops[j].stream, -1), j)
            w = set()
            for t, j in latest.items():
                if clock[s][t] >= j:
                    continue                 # already ordered behind it
                w.add(j)
                for u in range(ns):
                    clock[s][u] = max(clock[s][u], snap[j][u])
            clock[s][s] = i
            snap[i] = list(clock[s])
            need.update(w)
            waits.append(sorted(w))
            for t in op.writes:
                last[t] = i
        return waits, need

    def _compile(self, ops: List[Launch], recorded) -> C.c_void_p:
        """Compile an op list into a native program (csrc/program.hip)."""
        waits, need = self._schedule(ops, recorded)
        arr = (capi.Op * max(len(ops), 1))()
        for i, op in enumerate(ops):
            o = arr[i]
            o.kind, o.stream, o.desc = capi.OP_KIND[op.name], op.stream, C.addressof(op.desc)
            assert len(waits[i]) <= 8, "op waits on more than 8 producers"
            o.nwait = len(waits[i])
            for j, wv in enumerate(waits[i]):
                o.wait[j] = wv
            o.record = int(i in need)
        h = C.c_void_p()
        capi.call("stl_program_create", arr, len(ops), self.nstreams, C.byref(h))
        self._keep.append(arr)
        return h

    def _program(self, which: str) -> C.c_void_p:
        """The forward ("fwd") or backward ("bwd") program, compiled once; the backward one records an event at the last
        op of every gradient bucket (bucket_wait)."""
        if which not in self._progs:
            self._progs[which] = (self._compile(self.fwd_ops, ()) if which == "fwd" else
                                  self._compile(self.bwd_ops, [b.op for b in self.buckets]))
        return self._progs[which]

    def _run(self, h, stream: int, on_bucket=None):
        """Replay a native program on `stream` and the side streams.  With several streams the independent branches of
        each exchange module (and, in backward, the weight gradients) run concurrently; fork/join and cross-stream
        dependencies are HIP events inside stl_program_run.  on_bucket (the backward program): issue it range by range
        (stl_program_run_range) and call on_bucket(i) right after gradient bucket i's last op has been enqueued."""
        if self._side is None:
            self._make_streams()
        self._stream_arr[0] = stream
        if on_bucket is None:
            if self.lib.stl_program_run(h, self._stream_arr) != 0:
                raise RuntimeError(f"stl_program_run: {self.lib.stl_last_error().decode()}")
            return
        first = 0
        for i, b in enumerate(self.buckets):   # in op order: buckets are emitted as they close
            capi.call("stl_program_run_range", h, self._stream_arr, first, b.op + 1)
            first = b.op + 1
            on_bucket(i)
        capi.call("stl_program_run_range", h, self._stream_arr, first, len(self.bwd_ops))

    def _make_streams(self):
        """HIP streams of the program: index 0 is the caller's stream, 1 .. nstreams-1 the other branch streams.
        ONE set of side streams per device, shared by every engine (engines never run concurrently): each new HIP stream is
        another hardware queue, queues are spread round-robin over the four compute pipes, and two ACTIVE queues on one pipe
        are time-sliced -- a second engine with streams of its own ran its plan at half speed (W32 256x192 as the second
        plan of a process: 20.8 ms per step instead of 10.2).  (CU-masked streams and HIP stream priorities were measured
        in round 3 -- 27-92 ms resp. 14.64-14.76 vs 14.66 ms per step -- and removed.)"""
        n = self.nstreams
        self._stream_arr = (C.c_void_p * n)()
        self._side = []
        pool = _STREAM_POOL.setdefault(self.dev.index, {})
        with torch.cuda.device(self.dev):
            for i in range(1, n):
                if i not in pool:
                    s_ = torch.cuda.Stream(device=self.dev)
                    pool[i] = (s_, s_.cuda_stream)
                self._side.append(pool[i][0])
                self._stream_arr[i] = pool[i][1]

    def prep_weights(self, stream: int):
        st = self.store
        capi.call("stl_weight_prep", capi.dt2(self.dtype, self.fdtype), st.master.data_ptr(), self.wk.data_ptr(), self._wprep_tab.data_ptr(),
                  self._wprep_n, self._wprep_blocks, stream)

    def forward(self, stream: int, update_running: bool = True):
        """weights -> kernel layout, zero statistics, forward program, running-stat update."""
        self.generation += 1   # every pass overwrites the plan's activations (hrnet._Fn stale-backward check)
        self.prep_weights(stream)
        if self.training:
            self.stats.zero_()
        self._run(self._program("fwd"), stream)
        if self.training and update_running:
            st = self.store
            capi.call("stl_bn_running_update", self.stats.data_ptr(), st.bufs.data_ptr(), st.nbt.data_ptr(),
                      self._bn_tab.data_ptr(), len(self.bns), MOMENTUM, self.overflow.data_ptr(), stream)

    NO_OVERFLOW = 2 ** 31 - 1

    def check_forward_range(self):
        """Raise if a forward pass since the last call stored a non-finite raw conv output (one 4-byte read: call it where the
        host reads the loss anyway).  Training mode only: the guard rides on the BatchNorm statistics (stl_bn_running_update)."""
        i = int(self.overflow.item())
        if i == self.NO_OVERFLOW:
            return
        self.overflow.fill_(self.NO_OVERFLOW)
        bn = self.bns[i]
        name = next((k for k, off in self.store.param_off.items() if off == bn.param_off), f"BatchNorm #{i}")
        what = {capi.F16: "f16 (|y| > 65504)", capi.BF16: "bf16", capi.F32: "fp32"}[self.fdtype]
        raise FloatingPointError(
            f"stlpose_amd: the raw output of the convolution in front of {name[:-len('.weight')] if name.endswith('.weight') else name} "
            f"left the range of its {what} storage (non-finite BatchNorm statistics; first such layer in forward order).  "
            "The optimiser skipped that step (and skips every step until this is reported): the weights are intact; the running "
            "statistics of the layers behind it took their momentum update from the poisoned pass.  Forward tensors of the default "
            "'mixed' mode are f16; for a checkpoint with badly scaled weights use compute_dtype='bf16' (same speed, bf16 range) "
            "or 'fp32'.")

    def backward(self, stream: int, on_bucket=None):
        """expects self.dout filled; leaves dL/dparam in store.grads (overwrites; training plans) and, with input_grad, dL/d(img)
        in self.dimg (an eval plan writes nothing else that outlives the call).  on_bucket(i): called on the host right after
        gradient bucket i's last op has been ENQUEUED (the program is issued range by range, stl_program_run_range): the
        data-parallel path enqueues the bucket's all-reduce there, so that in every in-order hardware queue it sits directly
        behind the bucket instead of behind the rest of backward."""
        assert self.training or self.input_grad
        if self.training:   # (eval + input_grad: dimg only; rstats stays zero, the reductions go to the sink)
            self.rstats.zero_()
        # includes the per-bucket slab reductions and BatchNorm gradients
        self._run(self._program("bwd"), stream, on_bucket if self.buckets else None)

    def bucket_wait(self, i: int, stream: int):
        """Make `stream` wait until gradient bucket i (self.buckets[i]: flat slice [lo, hi)) of the
        backward pass enqueued last is final."""
        capi.call("stl_program_wait_op", self._program("bwd"), self.buckets[i].op, stream)


_STREAM_POOL: Dict[int, Dict] = {}   # device index -> {stream index: (owner object, hipStream_t)}


def bn_weight_keys(reg: Registry) -> set:
    """Keys of the BatchNorm scale parameters of `reg` (every ``<bn>.weight`` whose ``<bn>.running_mean`` is a buffer).
    Computed from the registry itself on every call.  Rounds 2-4 cached this set in a module-level dict keyed by ``id(reg)``:
    a Registry is created per model, CPython hands a collected registry's address to the next one, and a W32 model built
    after a ``tiny`` model had been dropped got the TINY key set -- its statistics arenas came out 512 KB short, the
    producers' atomics of the layers beyond the end landed in whatever followed (and were never zeroed): the one-in-five
    "output 0.39 off, NaN gradients" failure of the 12th GPU test of round 4 (tests/test_host_cpu.py)."""
    return {k[: -len("running_mean")] + "weight" for k, _ in reg.buffers if k.endswith("running_mean")}


def bn_stat_elems(reg: Registry) -> int:
    """fp64 elements of one statistics arena: [NSHARD][2C] per BatchNorm layer."""
    keys = bn_weight_keys(reg)
    return sum(int(math.prod(s)) for k, s in reg.params if k in keys) * 2 * capi.NSHARD


def _to_device(ctab, device) -> torch.Tensor:
    raw = bytes(ctab)
    t = torch.frombuffer(bytearray(raw), dtype=torch.uint8).clone()
    return t.to(device)
