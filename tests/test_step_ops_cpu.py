"""CPU: the yardsticks of tests/step_ops_ref.py are what they claim to be -- torch.optim, nn.BatchNorm2d, the header's index
formulas, the two summation orders of reduce_slabs_kernel, conv2d's autograd, PersonMSELoss -- and the bounds the GPU tests
apply would notice the faults they are there for (a dropped optimiser term, one shard read, a dropped slab, another order)."""
import math

import numpy as np
import pytest
import torch

from tests import step_ops_ref as R

F64, F32 = torch.float64, torch.float32


# ------------------------------------------------------------------------------------------------ optimisers
def torch_optim_run(kind, h, p, grads):
    """torch.optim in float64 on the same inputs (gradient times gscale first); the states after each step."""
    lr, b1, b2, eps, wd, mu, nest, gs = (float(x) for x in h)
    q = p.double().clone().requires_grad_(True)
    if kind == "adam":
        opt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    else:
        opt = torch.optim.SGD([q], lr=lr, momentum=mu, dampening=0, nesterov=bool(nest), weight_decay=wd)
    out = []
    for g in grads:
        q.grad = g.double() * gs
        opt.step()
        st = opt.state[q]
        if kind == "adam":
            out.append((q.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()))
        else:
            out.append((q.detach().clone(), st["momentum_buffer"].clone() if mu else None))
    return out


@pytest.mark.parametrize("name,kind,h", R.OPT_CONFIGS, ids=[c[0] for c in R.OPT_CONFIGS])
def test_optimiser_restatement_is_torch_optim_in_float64(name, kind, h):
    p, grads, stale = R.opt_data(255)
    ours, theirs = R.opt_run(kind, h, p, grads, stale, F64), torch_optim_run(kind, h, p, grads)
    assert len(ours) == R.OPT_STEPS == 4
    for a, b in zip(ours, theirs):
        for x, y in zip(a, b):
            if y is not None:   # (no momentum: torch keeps no buffer)
                assert R.rel_err(x, y) < 1e-13, name   # the same formula; torch fuses some of the operations


@pytest.mark.parametrize("name,kind,h", R.OPT_CONFIGS, ids=[c[0] for c in R.OPT_CONFIGS])
def test_a_dropped_optimiser_term_is_100_bounds_away(name, kind, h):
    p, grads, stale = R.opt_data(10007)
    y64, y32 = R.opt_run(kind, h, p, grads, stale, F64), R.opt_run(kind, h, p, grads, stale, F32)
    muts = R.mutations_of(kind, h)
    assert set(muts) <= set(R.MUTATIONS)
    for drop in muts:
        bad = R.opt_run(kind, h, p, grads, stale, F64, drop=drop)
        worst = 0.0
        for sb, s64, s32 in zip(bad, y64, y32):
            for xb, x64, x32 in zip(sb, s64, s32):
                worst = max(worst, R.rel_err(xb, x64) / R.bound(R.rel_err(x32, x64)))
        print(f"{name}: without {drop} the result moves by {worst:.0f} bounds")
        assert worst >= 100, (name, drop, worst)


def test_every_mutation_is_active_somewhere():
    seen = set()
    for _, kind, h in R.OPT_CONFIGS:
        seen |= set(R.mutations_of(kind, h))
    assert seen == set(R.MUTATIONS)
    assert R.OPT_SIZES[-1] == 4096 * 256 + 257   # nblocks_for(n, 256, 4096): 4096 blocks of 256 threads, then a second trip


# ------------------------------------------------------------------------------------------------ BatchNorm bookkeeping
MOM = float(np.float32(0.1))   # the float the C ABI receives


@pytest.mark.parametrize("count", list(R.BN_COUNTS))
def test_bn_reference_is_batchnorm2d_in_float64(count):
    b, h, w = R.BN_COUNTS[count]
    for x in R.bn_data(count):
        c = x.shape[1]
        g = torch.Generator().manual_seed(c)
        rm, rv = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
        nm, nv = R.bn_running_ref(x, rm, rv, MOM)
        if b * h * w == 1:   # torch refuses one value per channel; the variance of one value is 0, biased or not
            assert torch.equal(nv, (1 - MOM) * rv.double()) and torch.equal(nm, (1 - MOM) * rm.double() + MOM * x[0])
            continue
        bn = torch.nn.BatchNorm2d(c, momentum=MOM).double().train()
        bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
        bn(x.view(b, h, w, c).permute(0, 3, 1, 2).contiguous())
        assert R.rel_err(nm, bn.running_mean) < 1e-13 and R.rel_err(nv, bn.running_var) < 1e-13
        assert int(bn.num_batches_tracked) == 1
        if c == 48:
            assert nv[7] == (1 - MOM) * float(rv[7])                       # the constant channel
            assert (x[:, 5].mean() / x[:, 5].std()).item() > 20              # mean / std about 30


def test_bn_sums_need_every_shard_and_the_bound_sees_a_missing_one():
    assert 1.0 / float(np.float32(1.0 / 105)) != 105.0          # the kernel's rebuilt count is not the count
    for x in R.bn_data("3x7x5"):
        st = R.bn_sums(x)
        n, c = x.shape
        assert st.shape == (R.NSHARD, 2, c) and st[0].abs().min() > 0 and st[1].abs().min() > 0
        assert torch.allclose(st.sum(0)[0], x.sum(0), rtol=1e-13) and torch.allclose(st.sum(0)[1], (x * x).sum(0), rtol=1e-13)
        rm, rv = torch.zeros(c), torch.ones(c)
        nm, nv = R.bn_running_ref(x, rm, rv, MOM)
        bm, bv = R.bn_running_bound(x, nm, nv, MOM)
        for k in range(R.NSHARD):   # a kernel that reads one shard
            mean = st[k, 0] / n
            one = (1 - MOM) * rm.double() + MOM * mean
            assert ((one - nm).abs() / bm).max() > 100
        assert (bm > 0).all() and (bv > 0).all() and (bm <= 2e-7 * (nm.abs() + x.mean(0).abs())).all()


# ------------------------------------------------------------------------------------------------ stl_weight_prep
def tile_path(r) -> bool:
    """weight_prep_kernel's condition for the 32 x 32 tile path."""
    t = r["ks"] ** 2
    return (not r["patch"] and r["Ci"] % 4 == 0 and r["Co"] % 4 == 0 and t <= 9 and r["Cip"] == r["Ci"] and r["fwd_off"] % 4 == 0
            and (r["bwd_off"] < 0 or r["bwd_off"] % 4 == 0))


def test_weight_prep_table_reaches_every_path():
    rows, nsrc, nwk, nblk = R.wprep_layout()
    assert [tile_path(r) for r in rows] == [True, True, False, True, False, False, False, True]
    assert rows[3]["src_off"] % 4 != 0 and tile_path(rows[3])                    # the row-walk load
    assert rows[4]["fwd_off"] % 4 != 0 and rows[5]["Cip"] != rows[5]["Ci"]        # two ways onto the generic path
    assert rows[2]["Ci"] % 4 != 0
    assert rows[6]["patch"] and rows[6]["bwd_off"] >= 0 and rows[6]["Cip"] == 32
    assert rows[7]["bwd_off"] < 0
    r = rows[0]   # 36 -> 36, 1x1: four partial tiles on two blocks
    assert -(-r["Co"] // 32) * -(-r["Ci"] // 32) == 4 and rows[1]["blk0"] - r["blk0"] == 2
    assert nblk == sum(-(-r["Co"] * r["Ci"] * r["ks"] ** 2 // 1024) for r in rows)
    assert all(rows[i]["blk0"] < rows[i + 1]["blk0"] for i in range(len(rows) - 1))


@pytest.mark.parametrize("gd,fd", [(F32, F32), (torch.bfloat16, torch.bfloat16), (torch.float16, torch.float16), (torch.bfloat16, torch.float16)])
def test_weight_prep_reference_is_the_headers_index_formula(gd, fd):
    rows, nsrc, nwk, nblk = R.wprep_layout()
    master = torch.randn(nsrc, generator=torch.Generator().manual_seed(3))
    sent = 0x5A5A5A5A if gd == F32 else 0x5A5A
    wk = R.wprep_ref(master, rows, nwk, gd, fd, sent)
    it = wk.dtype
    exp = torch.full((nwk,), sent, dtype=it)
    written = 0
    for r in rows:
        co, ci, ks, cip = r["Co"], r["Ci"], r["ks"], r["Cip"]
        t = ks * ks
        w = master[r["src_off"]:r["src_off"] + co * ci * t].view(co, ci, t)
        wf, wg = w.to(fd).view(it), w.to(gd).view(it)
        for o in range(co):
            for c in range(ci):
                for tap in range(t):
                    if r["patch"]:
                        exp[r["fwd_off"] + o * cip + tap * ci + c] = wf[o, c, tap]
                        exp[r["bwd_off"] + (tap * ci + c) * co + o] = wg[o, c, tap]
                    else:
                        exp[r["fwd_off"] + (o * t + tap) * cip + c] = wf[o, c, tap]
                        if r["bwd_off"] >= 0:
                            exp[r["bwd_off"] + (c * t + (t - 1 - tap)) * co + o] = wg[o, c, tap]
        written += co * ci * t * (2 if r["bwd_off"] >= 0 else 1)
    assert torch.equal(wk, exp)
    assert int((wk != sent).sum()) >= written - 8   # the layouts do not overlap (a value may happen to equal the sentinel)
    if gd != fd:   # the two 16-bit types round differently: a layout written in the other type would show
        r = rows[1]
        w = master[r["src_off"]:r["src_off"] + r["Co"] * r["Ci"] * 9]
        assert not torch.equal(w.to(gd).view(it), w.to(fd).view(it))


# ------------------------------------------------------------------------------------------------ stl_reduce_slabs
@pytest.mark.parametrize("nsplit", R.SLAB_NSPLIT)
def test_slab_orders_differ_and_a_dropped_slab_shows(nsplit):
    rows, npart, ngrad, nblk = R.slab_layout(nsplit)
    partials = R.slab_partials(rows, npart)
    assert [R.slab_is_vector(r) for r in rows] == [True, True, False, False, True]
    assert torch.isnan(partials).any()
    for r in rows:
        assert r["part_off"] % 4 == 0 and r["stride"] % 4 == (0 if R.slab_is_vector(r) else r["stride"] % 4)
        if r["pad"]:
            assert r["pad"] > r["Co"] * r["ks"] ** 2 * r["Ci"]
        terms = R.slab_terms(partials, r)
        assert terms.shape == (nsplit, r["Co"], r["Ci"], r["ks"], r["ks"]) and not torch.isnan(terms).any()
        a, b = R.sum_in_slab_order(terms), R.sum_pairwise_by_eight(terms)
        y64 = terms.double().sum(0)
        for s in (a, b):   # both orders are sums: within the fp64 bound
            assert R.rel_err(s, y64) <= R.bound(R.rel_err(terms.sum(0), y64))
        if nsplit < 8:
            assert torch.equal(a, b)            # no full group of eight: one order
        elif r["Co"] * r["Ci"] >= 100:
            assert not torch.equal(a, b)        # the orders differ in bits on this data
        if nsplit > 1 and r["Co"] * r["Ci"] >= 100:
            for k in (0, nsplit - 1, min(7, nsplit - 1)):
                less = torch.cat([terms[:k], terms[k + 1:]])
                assert not torch.equal(R.sum_in_slab_order(less), a) and not torch.equal(R.sum_pairwise_by_eight(less), b)
    full = R.slab_ref(partials, rows, ngrad)
    part = R.slab_ref(partials, rows, ngrad, only=(1, 2))
    assert int((full == R.SLAB_SENTINEL).sum()) == 3 * (len(rows) + 1) - 3 + 3   # the gaps, nothing else
    r1, r3 = rows[1], rows[3]
    assert torch.equal(part[r1["grad_off"]:r3["grad_off"] - 3], full[r1["grad_off"]:r3["grad_off"] - 3])
    assert (part[:r1["grad_off"]] == R.SLAB_SENTINEL).all() and (part[r3["grad_off"] - 3:] == R.SLAB_SENTINEL).all()


# ------------------------------------------------------------------------------------------------ head and loss
def test_head_reference_is_the_matrix_product():
    x, w, bias, dout = R.head_data(17, 48, "306", torch.bfloat16)
    assert torch.equal(x, x.bfloat16().float())
    out, dx, dw, db = R.head_ref(x, w, bias, dout)
    xd, wd, dd = x.double(), w.double(), dout.double()
    assert R.rel_err(out, torch.einsum("bchw,jc->bjhw", xd, wd) + bias.double().view(1, -1, 1, 1)) < 1e-14
    assert R.rel_err(dx, torch.einsum("bjhw,jc->bchw", dd, wd)) < 1e-14
    assert R.rel_err(dw, torch.einsum("bjhw,bchw->jc", dd, xd)) < 1e-13
    assert R.rel_err(db, dd.sum((0, 2, 3))) < 1e-13
    b, h, ww = R.HEAD_PIXELS["105"]
    assert b * h * ww == 105 < 256 and math.prod(R.HEAD_PIXELS["306"]) == 306 and 306 % 256 != 0


def test_mse_reference_is_the_closed_form():
    o, t, tw = R.mse_data(3, 17, 35)
    loss, dout = R.mse_ref(o, t, tw, 0.25)
    n = o.numel()
    d = (o.double() - t.double()) * tw.double()
    assert abs(loss.item() - 0.5 * (d * d).mean().item()) < 1e-15
    assert R.rel_err(dout, d * tw.double() / n * 0.25) < 1e-14
    assert (dout[0, 1] == 0).all() and tw[0, 1] == 0
