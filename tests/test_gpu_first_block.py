"""The folded critic first block (csrc/first_block.hip) through the C ABI -- ngan_first_block_fwd, _bwd, _dx and the two size queries --
kernel by kernel and per element against fp64, at the smallest shapes that reach every special case of the file: W = 1, 2, 3 and the
workgroup span - 1, + 0, + 1 (both column masks on one pixel; a second x-block whose padding lanes share a DPP row with live ones),
H = 1, 2, 7, 8, 9, 17 (one-row images, a halo row owned by the neighbouring chunk on either side), B = 1 and 3, C = 1, 16, 20, 64 (the
finish kernel's guarded second 16-channel pass, FB_MAX_C), N = 16 and 32 (PW = 16 and 8), each of bf, b_conv, gbf, gb_conv null, every
accumulate bit alone, none, all and bits set for null outputs, pool 0 and 1, and the sums plan at R = 8 with exactly 1024 slabs,
R = 16, R = 32 and two x-blocks with R = 16.

Per element   |got - ref| <= n_round 2^-23 |ref| + C_ACC 2^-24 absref + carried,   C_ACC = 8,   n_round, absref and the carried bound
of the folded tables / pixel sums derived per output in tests/first_block_cases.py.  The constants were settled on the CPU against fp32
emulations in the kernels' summation order (tests/test_first_block_bounds_cpu.py: every emulated ratio <= 0.5; one raise, the folded
tables -> C_ACC 16), never against a kernel.  Every output starts as NaN between guard planes of a sentinel: an element no thread wrote
fails the comparison, and so does a store outside the tensor (y, rnorm: one sample on each side; gx: a 2H x 2W plane, which covers the
pooled form; the workspace past ngan_first_block_workspace_floats and the tables past ngan_first_block_table_floats).  A second launch
of every entry point on the same operands is bit-equal (no atomics in this file).

What ngan_first_block_bwd leaves behind its slabs are the reduced pixel sums S1 / S0 (not the folded tables A / Bv, which only the
forward computes): they are pinned against fp64 as output "S".

measured on MI355X (a record, not a bound: worst err / bound per output over all cases and the case that gave it, the emulation's figure
for the same case in brackets; 1 is the bound): tables 0.291 (0.291) at (3, 7, 33, 16, 32), with C_ACC 16; y 0.080 (0.080) and rnorm
0.069 (0.069) at (3, 9, 65, 1, 16); S 0.232 (0.232) at (1, 17, 2, 64, 32); gW 0.193 (0.193) at (1, 8, 2, 64, 32), accumulated 0.038
(0.038); gwf 0.046 (0.046) at (1, 1, 3, 20, 16), accumulated 0.002 (0.002); gbf 0.030 (0.030) at (1, 1, 1, 1, 16), accumulated 0.002
(0.002); gbc 0.173 (0.173) at (1, 9, 3, 20, 32), accumulated 0.013 (0.013); gx plain and pooled 0.034 (0.034) at (1, 1, 64, 1, 16); the
sums plan cases S 0.011 at 1024 slabs of R = 8, 0.010 at R = 16, 0.007 at R = 32, 0.003 at two x-blocks with R = 16; the operator-level
.grad test 0.037 / 0.002 / 0.002 / 0.026.  The parameter gradients sit far below their bound because most of it is the carried bound
of S1 / S0, a worst case over every pixel of the batch.  The first run measured y 0.080 where the emulation said 0.073: the forward's
f4dot(acc, acc) compiles to four rounded squares added in order, not to the fma chain the image gradient's f4dot becomes; the
emulation was corrected, no constant moved and no kernel needed a fix.  No guard was touched and no element left unwritten.  The module
takes 6 s."""
import numpy as np
import pytest
import torch

import first_block_cases as F
from test_gpu_ops import DEV

pytestmark = pytest.mark.gpu
SLOPE, EPS = F.SLOPE, F.EPS
SENTINEL = 7.0
SMALL_GUARD = 64
BITS = {"gW": 1, "gwf": 2, "gbf": 4, "gbc": 8}


def dv(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().float().cpu().numpy()


class Guarded:
    """a tensor of `shape` between two guard runs of `guard` sentinel elements; `fill`: a host array, or None for NaN"""

    def __init__(self, shape, guard, fill=None):
        n = int(np.prod(shape))
        self.full = torch.full((n + 2 * guard,), SENTINEL, device=DEV, dtype=torch.float32)
        self.t = self.full[guard:guard + n].view(*shape)
        self.t.copy_(dv(fill)) if fill is not None else self.t.fill_(float("nan"))
        self.guard = guard

    def intact(self):
        g = self.guard
        return bool((self.full[:g] == SENTINEL).all()) and bool((self.full[self.full.numel() - g:] == SENTINEL).all())


class Checker:
    """collects err / bound of every output of one test and asserts at the end, so that one run shows every figure"""

    def __init__(self, case):
        self.case, self.bad = case, []

    def __call__(self, name, got, entry, tag=""):
        worst = F.worst(host(got), entry, name)
        print(f"STAT first_block {name}{tag} {self.case}: {worst:.3f}")
        if not worst <= 1.0:
            self.bad.append((name + tag, worst))

    def guards(self, **bufs):
        for k, b in bufs.items():
            if b is not None and not b.intact():
                self.bad.append((k, "guard touched"))

    def done(self):
        assert not self.bad, (self.case, self.bad)


def run_fwd(ngan, case, bf_null=False, bc_null=False):
    """one ngan_first_block_fwd launch into guarded NaN buffers -> (y, rnorm, tables) as Guarded"""
    B, H, Wd, C, N = case
    d = F.inputs(*case)
    nt = ngan._C.lib().ngan_first_block_table_floats(N)
    assert nt == 2 * 9 * N
    y, rn, tab = Guarded((B, H, Wd, N), H * Wd * N), Guarded((B, H, Wd), H * Wd), Guarded((2, 9, N), 4096)
    ngan._C.call("ngan_first_block_fwd", dv(d["p"]), dv(d["w"]), dv(d["wf"]), None if bf_null else dv(d["bf"]),
                 None if bc_null else dv(d["bc"]), y.t, rn.t, tab.t, B, H, Wd, C, N, d["scale"], SLOPE, EPS)
    return y, rn, tab


def check_fwd(ngan, case, ck, bf_null=False, bc_null=False, tag=""):
    d = F.inputs(*case)
    bf, bc = (None if bf_null else d["bf"]), (None if bc_null else d["bc"])
    y, rn, tab = run_fwd(ngan, case, bf_null, bc_null)
    ck.guards(y=y, rnorm=rn, tables=tab)
    ck("tables", tab.t, F.tables_ref(d["w"], d["wf"], bf, d["scale"])["tables"], tag)
    ref = F.fwd_ref(d["p"], d["w"], d["wf"], bf, bc, d["scale"], host(y.t))
    ck("y", y.t, ref["y"], tag)
    ck("rnorm", rn.t, ref["rnorm"], tag)
    if F.sign_violations(*ref["_pre"], host(y.t)):
        ck.bad.append(("LeakyReLU sign against a decided fp64 pre-activation", F.sign_violations(*ref["_pre"], host(y.t))))
    if bf_null and not bool((tab.t[1] == 0).all()):
        ck.bad.append(("Bv with bf null", "not zero"))
    y2, rn2, tab2 = run_fwd(ngan, case, bf_null, bc_null)
    if not (torch.equal(y.t, y2.t) and torch.equal(rn.t, rn2.t) and torch.equal(tab.t, tab2.t)):
        ck.bad.append(("fwd", "second launch differs"))
    return tab


def run_bwd(ngan, case, mask=0, bf_null=False, gbf_null=False, gbc_null=False):
    """one ngan_first_block_bwd launch -> ({output: Guarded or None}, workspace Guarded); an output whose bit is set starts from its
    buffer, every other one as NaN"""
    B, H, Wd, C, N = case
    d = F.inputs(*case)
    nws = ngan._C.lib().ngan_first_block_workspace_floats(B, H, N)
    assert nws == (F.MAX_SLABS + 1) * 2 * 9 * N
    bufs = {"gW": d["bufW"], "gwf": d["bufwf"], "gbf": d["bufbf"], "gbc": d["bufbc"]}
    null = {"gbf": gbf_null, "gbc": gbc_null}
    out = {k: None if null.get(k) else Guarded(v.shape, SMALL_GUARD, v if mask & BITS[k] else None) for k, v in bufs.items()}
    ws = Guarded((nws,), 4096)
    t = lambda g: None if g is None else g.t
    ngan._C.call("ngan_first_block_bwd", dv(d["p"]), dv(d["gc"]), dv(d["w"]), dv(d["wf"]), None if bf_null else dv(d["bf"]),
                 t(out["gW"]), t(out["gwf"]), t(out["gbf"]), t(out["gbc"]), ws.t, B, H, Wd, C, N, d["scale"], mask)
    return out, ws


def check_bwd(ngan, case, ck, mask=0, bf_null=False, gbf_null=False, gbc_null=False, tag=""):
    B, H, Wd, C, N = case
    d = F.inputs(*case)
    bufs = {"gW": d["bufW"], "gwf": d["bufwf"], "gbf": d["bufbf"], "gbc": d["bufbc"]}
    out, ws = run_bwd(ngan, case, mask, bf_null, gbf_null, gbc_null)
    ck.guards(workspace=ws, **out)
    ref = F.bwd_ref(d["p"], d["gc"], d["w"], d["wf"], None if bf_null else d["bf"], d["scale"])
    S = ws.t[F.MAX_SLABS * 18 * N:].view(2, 9, N)
    ck("S", S, ref["S"], tag)
    slabs = F.plan(*case)[3]
    if bool(torch.isnan(ws.t[:slabs * 18 * N]).any()):
        ck.bad.append(("slabs", "unwritten"))
    for k, g in out.items():
        if g is not None:
            ck(k, g.t, F.plus(ref[k], bufs[k]) if mask & BITS[k] else ref[k], (" acc" if mask & BITS[k] else "") + tag)
    out2, ws2 = run_bwd(ngan, case, mask, bf_null, gbf_null, gbc_null)
    same = torch.equal(S, ws2.t[F.MAX_SLABS * 18 * N:].view(2, 9, N))
    if not (same and all(torch.equal(out[k].t, out2[k].t) for k in out if out[k] is not None)):
        ck.bad.append(("bwd", "second launch differs"))


def run_dx(ngan, case, tables, pool):
    B, H, Wd, C, N = case
    gx = Guarded((B, 2 * H, 2 * Wd) if pool else (B, H, Wd), 4 * H * Wd)
    ngan._C.call("ngan_first_block_dx", dv(F.inputs(*case)["gc"]), tables, gx.t, B, H, Wd, N, pool)
    return gx


def check_dx(ngan, case, ck, tables):
    d = F.inputs(*case)
    for pool in (0, 1):
        gx = run_dx(ngan, case, tables, pool)
        ck.guards(gx=gx)
        ck("gx", gx.t, F.dx_ref(d["gc"], d["w"], d["wf"], d["scale"], pool)["gx"], " pooled" if pool else "")
        if not torch.equal(gx.t, run_dx(ngan, case, tables, pool).t):
            ck.bad.append(("dx", "second launch differs"))


@pytest.mark.parametrize("case", F.FULL)
def test_first_block_edges_against_fp64(ngan, case):
    """fwd (tables, y, rnorm), bwd (S, gW, gwf, gbf, gbc, written) and dx (plain and pooled, on the tables the forward wrote) of one
    shape: bounds, guards, unwritten elements, LeakyReLU signs, bit-equal second launches"""
    ck = Checker(case)
    tab = check_fwd(ngan, case, ck)
    check_bwd(ngan, case, ck)
    check_dx(ngan, case, ck, tab.t)
    ck.done()


@pytest.mark.parametrize("case", F.PLAN_CASES)
def test_first_block_sums_plan_against_fp64(ngan, case):
    """ngan_first_block_bwd where the sums launch takes more than 8 rows per workgroup, and at exactly 1024 slabs"""
    assert ngan._C.first_block_plan(*case) == (0, F.PLAN_EXPECT[case])
    ck = Checker(case)
    check_bwd(ngan, case, ck)
    ck.done()


@pytest.mark.parametrize("which", F.NULLS)
@pytest.mark.parametrize("case", F.NULL_SHAPES)
def test_first_block_null_arguments(ngan, case, which):
    """bf, b_conv, gbf and gb_conv each null in turn; with bf null the Bv table is exactly zero"""
    ck = Checker((case, which + " null"))
    if which in ("bf", "bc"):
        check_fwd(ngan, case, ck, bf_null=which == "bf", bc_null=which == "bc")
    if which != "bc":
        check_bwd(ngan, case, ck, bf_null=which == "bf", gbf_null=which == "gbf", gbc_null=which == "gbc")
    ck.done()


@pytest.mark.parametrize("mask,gbf_null,gbc_null", F.ACCUMULATE)
@pytest.mark.parametrize("case", F.NULL_SHAPES)
def test_first_block_accumulate_bits(ngan, case, mask, gbf_null, gbc_null):
    """each accumulate bit steers its own output: old + fresh where the bit is set (buffers of the size of the gradient), written
    elsewhere (from NaN), and a bit set for a null output is ignored"""
    ck = Checker((case, mask, gbf_null, gbc_null))
    check_bwd(ngan, case, ck, mask=mask, gbf_null=gbf_null, gbc_null=gbc_null)
    ck.done()


REFUSED = [((1025, 1, 1, 16, 16), r"needs 1025 slabs \(max 1024\)"), ((2, 8, 8, 65, 16), "unsupported"), ((2, 8, 8, 16, 8), "unsupported"),
           ((2, 8, 8, 16, 64), "unsupported")]


@pytest.mark.parametrize("shape,message", REFUSED)
def test_first_block_refusals_write_nothing(ngan, shape, message):
    """a shape the plan refuses: every entry point raises with the library's message before anything is launched"""
    B, H, Wd, C, N = shape
    assert ngan._C.first_block_plan(*shape)[0] == F.NGAN_ERR_SHAPE
    d = F.draws(5, p=(B, H, Wd), w=(N, C, 3, 3), wf=(C,), bf=(C,), bc=(N,), gc=(B, H, Wd, N))
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    y, rn, tab = nan(B, H, Wd, N), nan(B, H, Wd), nan(2 * 9 * N)
    with pytest.raises(RuntimeError, match=r"ngan_first_block_fwd failed with status -2: first_block_fwd: .*" + message):
        ngan._C.call("ngan_first_block_fwd", dv(d["p"]), dv(d["w"]), dv(d["wf"]), dv(d["bf"]), dv(d["bc"]), y, rn, tab, B, H, Wd, C, N,
                     0.1, SLOPE, EPS)
    gW, gwf, gbf, gbc, ws = nan(N, C, 3, 3), nan(C), nan(C), nan(N), nan((F.MAX_SLABS + 1) * 18 * N)
    with pytest.raises(RuntimeError, match=r"ngan_first_block_bwd failed with status -2: first_block_bwd: .*" + message):
        ngan._C.call("ngan_first_block_bwd", dv(d["p"]), dv(d["gc"]), dv(d["w"]), dv(d["wf"]), dv(d["bf"]), gW, gwf, gbf, gbc, ws,
                     B, H, Wd, C, N, 0.1, 0)
    outs = [y, rn, tab, gW, gwf, gbf, gbc, ws]
    if C <= F.FB_MAX_C:             # dx takes no C: a shape refused for its C alone is dx's to run
        gx = nan(B, 2 * H, 2 * Wd)
        with pytest.raises(RuntimeError, match=r"ngan_first_block_dx failed with status -2: first_block_dx: .*" + message):
            ngan._C.call("ngan_first_block_dx", dv(d["gc"]), tab, gx, B, H, Wd, N, 1)
        outs.append(gx)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs)


def test_first_block_backward_accumulates_into_existing_grads(ngan):
    """ops.FirstBlock.backward with a contiguous .grad on all four parameters (ops._small_grads_in_place, the default): every .grad keeps
    its buffer and holds old + fresh within the accumulate bound"""
    ops = ngan.ops
    assert ops._small_grads_in_place
    case = F.NULL_SHAPES[0]
    B, H, Wd, C, N = case
    d = F.inputs(*case)
    par = lambda a: torch.nn.Parameter(dv(a))
    wf, bf, w, bc = par(d["wf"].reshape(C, 1, 1, 1)), par(d["bf"]), par(d["w"]), par(d["bc"])
    bufs = {"gW": d["bufW"], "gwf": d["bufwf"], "gbf": d["bufbf"], "gbc": d["bufbc"]}
    params = {"gW": w, "gwf": wf, "gbf": bf, "gbc": bc}
    for k, p_ in params.items():
        p_.grad = dv(bufs[k]).reshape(p_.shape).contiguous()
    ptrs = {k: p_.grad.data_ptr() for k, p_ in params.items()}
    y, rn = ops.FirstBlock.apply(dv(d["p"]).unsqueeze(-1), wf, bf, w, bc, False, d["scale"], SLOPE, None)
    gy = dv(F.draws(9, gy=(B, H, Wd, N))["gy"])
    gc = torch.empty_like(y)         # the gradient at the pre-activation, as FirstBlock.backward forms it
    ngan._C.call("ngan_lrelu_pixelnorm_bwd", gy, None, y.detach(), rn, gc, B * H * Wd, N, SLOPE)
    y.backward(gy)
    ref = F.bwd_ref(d["p"], host(gc), d["w"], d["wf"], d["bf"], d["scale"])
    ck = Checker(case)
    for k, p_ in params.items():
        assert p_.grad.data_ptr() == ptrs[k], k
        ck(k, p_.grad.reshape(bufs[k].shape), F.plus(ref[k], bufs[k]), " acc .grad")
    ck.done()


def test_refused_critic_batch_takes_the_unfused_pair_and_trains(ngan, monkeypatch):
    """a critic batch the plan refuses (1026 samples of 16 x 16: one slab per sample at the least) runs FromImage + ConvLReLUPN, not the
    fold, and one critic step goes through; the same net on a batch the plan takes uses the fold"""
    ops = ngan.ops
    torch.manual_seed(2)
    D = ngan.models.Discriminator_PG([16, 32], image_size_init=8)
    D.set_resolution(16, 1.0)
    D.to(DEV)
    loss_fn = ngan.loss_functions.D_W_loss(None, D, 0.001)
    calls = []
    real_apply = ops.FirstBlock.apply
    monkeypatch.setattr(ops.FirstBlock, "apply", lambda *a: (calls.append(a[0].shape[0]), real_apply(*a))[1])
    small = torch.rand(4, 1, 16, 16, device=DEV) * 2 - 1
    loss_fn(small, fake_images=-small)[0].backward()
    assert calls == [8], "the fold did not run on a batch it takes"
    B = 513
    assert ngan._C.first_block_plan(2 * B, 8, 8, 16, 16)[0] == F.NGAN_ERR_SHAPE == ngan._C.first_block_plan(2 * B, 16, 16, 16, 16)[0]
    opt = torch.optim.Adam(D.parameters(), lr=1e-3)
    opt.zero_grad(set_to_none=True)
    before = [p.detach().clone() for p in D.parameters()]
    real = torch.rand(B, 1, 16, 16, device=DEV) * 2 - 1
    loss, _, _ = loss_fn(real, fake_images=real.flip(0) * 0.5)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert calls == [8], "the fold ran on a batch its plan refuses"
    assert bool(torch.isfinite(loss))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in D.parameters())
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, D.parameters()))
