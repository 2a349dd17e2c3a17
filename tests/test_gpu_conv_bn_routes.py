"""BatchNorm2d of the conv path (cgl_bn2d_* in csrc/cgl_conv_bn.hip) at the shapes and forms no other test reaches,
against fp64 F.batch_norm + autograd, with elementwise bounds in the form DESIGN.md 5a derived for BatchNorm1d.

What the cases are for (the launch record, conv_ops.last_launches, names the kernel that ran):
  * rows per call that are no power of two (hw 49, 9, 1 with 2 or 3 images per call: chan_chunk falls to chunks of
    2 and 1 rows), C 4 / 8 / 256, one and two stacked calls, eval mode;
  * nvalid (the short real batch) on every BatchNorm2d entry point: the reference is the BatchNorm over the valid
    images alone, padding images get a zero input gradient, the running variance is unbiased over the valid rows;
  * cgl_eltwise's wrap of its 8192-block grid (more than 2^21 float4s), the rows past the wrap checked by themselves;
  * cgl_chan_reduce, the 4-byte form of the channel reduction (CGL_CHAN_SCALAR=1, and the only form for the column
    sum of C 1 or 2), in every mode.  Its rows are split over 256 / C lanes per channel where cgl_chan_reduce4 uses
    1024 / C, so the two sum in different orders: each is held to the reference, and on integer data (every sum
    exact) they must agree to the bit;
  * cgl_colsum_k (column sums at a channel count that is no power of two) with a ragged last 32-row chunk;
  * the two entry points of a direction are one path: cgl_bn2d_fwd / cgl_bn2d_bwd leave their chunk partials in the
    workspace, and the _stats form given those partials must write the same bits from the same launches.

Bounds, u = 2^-24, sc = invstd gamma (the reductions accumulate in double, so only the fp32 roundings of the
finalize and the apply count):
  save_mean 2 u |mean|, save_invstd 2 u invstd, running statistics 2 u (|old| + |new term|) per stacked call;
  y:  16 u (|x sc| + |beta| + |mean sc| + |y|)                     (5a: sh = beta - mean sc32 is formed rounded);
  dX: 16 u (|g| + |S / n| + |(x - mean) D invstd^2 / n| + |mean D invstd^2 / n|) invstd |gamma|
      (5a's form; the last term is the fp32 rounding of save_mean, which the fp64 autograd reference does not have);
  dgamma: 8 u invstd (sum |(x - mean) g| + |mean| |S|);  dbeta: 8 u sum |g|.
The worst ratios are printed.
"""
import os

import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_stats_canary import canary_ok, padded

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
EPS, MOM, SLOPE = 0.8, 0.1, 0.2


def ops():
    from cglgan import conv_ops
    return conv_ops


def kernels():
    return [l.kernel for l in ops().last_launches()]


class scalar_reduce:
    """CGL_CHAN_SCALAR=1 for the block (read per launch)"""

    def __init__(self, on=True):
        self.on = on

    def __enter__(self):
        self.old = os.environ.get("CGL_CHAN_SCALAR")
        if self.on:
            os.environ["CGL_CHAN_SCALAR"] = "1"

    def __exit__(self, *a):
        if self.on:
            if self.old is None:
                os.environ.pop("CGL_CHAN_SCALAR", None)
            else:
                os.environ["CGL_CHAN_SCALAR"] = self.old


def make(n, hw, C, seed, ints=False):
    g = torch.Generator().manual_seed(seed)
    if ints:
        x = torch.randint(-2, 3, (n, hw, C), generator=g).float()
        dy = torch.randint(-2, 3, (n, hw, C), generator=g).float()
    else:
        x = (torch.randn(n, hw, C, generator=g) * 2 + 0.5).float()
        dy = torch.randn(n, hw, C, generator=g).float()
    gamma = ((0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.3, -1.0, 1.0)).float()
    beta = torch.randn(C, generator=g).float()
    rm = (0.1 * torch.randn(C, generator=g)).float()
    rv = (1 + 0.1 * torch.rand(C, generator=g)).float()
    return dict(x=x, dy=dy, gamma=gamma, beta=beta, rm=rm, rv=rv)


def ratio(got, ref, bound, what, rat):
    got = got.detach().double().cpu()
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    r = float(((got - ref).abs() / bound.clamp_min(1e-300)).max())
    rat[what] = max(rat.get(what, 0.0), r)


def fwd_ref(d, n, hw, C, groups, act, valid=None, train=True):
    """fp64 F.batch_norm per stacked call, in call order (call 0 over its first `valid` images only).
    Returns per-call (mean, invstd), y [n, hw, C] (padding images: NaN = unchecked), its bound, the running
    statistics and their bounds."""
    ng = n // groups
    x, gam, bet = d["x"].double(), d["gamma"].double(), d["beta"].double()
    rm, rv = d["rm"].double().clone(), d["rv"].double().clone()
    rmb, rvb = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    y = torch.full((n, hw, C), float("nan"), dtype=torch.float64)
    yb = torch.ones(n, hw, C, dtype=torch.float64)
    stats = []
    for q in range(groups):
        nq = valid if (q == 0 and valid is not None) else ng
        xq = x[q * ng:q * ng + nq]
        xf = xq.permute(0, 2, 1).reshape(nq, C, hw, 1)
        if train:
            rm0, rv0 = rm.clone(), rv.clone()
            o = F.batch_norm(xf, rm, rv, gam, bet, True, MOM, EPS)
            mean = xq.reshape(-1, C).mean(0)
            var = xq.reshape(-1, C).var(0, unbiased=False)
            rmb += 2 * U * ((1 - MOM) * rm0.abs() + (rm - (1 - MOM) * rm0).abs())
            rvb += 2 * U * ((1 - MOM) * rv0.abs() + (rv - (1 - MOM) * rv0).abs())
        else:
            o = F.batch_norm(xf, rm, rv, gam, bet, False, MOM, EPS)
            mean, var = rm, rv
        inv = 1.0 / torch.sqrt(var + EPS)
        sc = inv * gam
        o = o.reshape(nq, C, hw).permute(0, 2, 1)
        if act:
            o = torch.where(o > 0, o, o * float(torch.tensor(SLOPE, dtype=torch.float32)))
        y[q * ng:q * ng + nq] = o
        yb[q * ng:q * ng + nq] = 16 * U * ((xq * sc).abs() + bet.abs() + (mean * sc).abs() + o.abs())
        stats.append((mean, inv))
    return stats, y, yb, (rm, rmb), (rv, rvb)


def bwd_ref(d, n, hw, C, groups, g_of, valid=None):
    """fp64 autograd of F.batch_norm (train) per stacked call, upstream gradient g_of(call rows) (the LeakyReLU'
    already applied by the caller).  Returns dX (padding images: 0), its bound, dgamma, dbeta and their bounds."""
    ng = n // groups
    x, gam, bet = d["x"].double(), d["gamma"].double(), d["beta"].double()
    dx, dxb = torch.zeros(n, hw, C, dtype=torch.float64), torch.zeros(n, hw, C, dtype=torch.float64)
    dg, dgb = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    db, dbb = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    for q in range(groups):
        nq = valid if (q == 0 and valid is not None) else ng
        sl = slice(q * ng, q * ng + nq)
        xq = x[sl].reshape(-1, C).clone().requires_grad_(True)
        gq, bq = gam.clone().requires_grad_(True), bet.clone().requires_grad_(True)
        gu = g_of(sl).reshape(-1, C)
        F.batch_norm(xq, None, None, gq, bq, True, MOM, EPS).backward(gu)
        dx[sl] = xq.grad.reshape(nq, hw, C)
        dg += gq.grad
        db += bq.grad
        rows = nq * hw
        xd = xq.detach()
        mean = xd.mean(0)
        inv = 1.0 / torch.sqrt(xd.var(0, unbiased=False) + EPS)
        xc = xd - mean
        S, D = gu.sum(0), (xc * gu).sum(0)
        t = gu.abs() + (S / rows).abs() + (xc * D * inv * inv / rows).abs() + (mean * D * inv * inv / rows).abs()
        dxb[sl] = (16 * U * t * inv * gam.abs()).reshape(nq, hw, C)
        dgb += 8 * U * inv * ((xc * gu).abs().sum(0) + mean.abs() * S.abs())
        dbb += 8 * U * gu.abs().sum(0)
    return dx, dxb, (dg, dgb), (db, dbb)


def run_fwd(d, n, hw, C, groups, act, nv=None, train=True, scalar=False):
    O = ops()
    y, ybuf = padded(n * hw * C)
    y.fill_(float("nan"))
    rm, rv = d["rm"].to(DEV), d["rv"].to(DEV)
    sm, smbuf = padded(groups * C)
    si, sibuf = padded(groups * C)
    nvd = torch.tensor([nv], dtype=torch.int32, device=DEV) if nv is not None else None
    with scalar_reduce(scalar):
        O.bn2d_fwd(d["x"].to(DEV), n, hw, C, d["gamma"].to(DEV), d["beta"].to(DEV), y, groups=groups, eps=EPS,
                   momentum=MOM, running_mean=rm, running_var=rv, train=train, act=act, slope=SLOPE,
                   save_mean=sm if train else None, save_invstd=si if train else None, nvalid=nvd)
        ks = O.last_launches()
    torch.cuda.synchronize()
    for t, b, k in ((y, ybuf, "y"), (sm, smbuf, "save_mean"), (si, sibuf, "save_invstd")):
        canary_ok(b, t.numel(), k)
    return y.view(n, hw, C), rm, rv, sm.view(groups, C), si.view(groups, C), ks


def check_fwd(out, ref, n, hw, C, groups, rat, tag, valid=None, train=True):
    y, rm, rv, sm, si, _ = out
    stats, yr, yb, (rmr, rmb), (rvr, rvb) = ref
    ng = n // groups
    for q in range(groups):
        nq = valid if (q == 0 and valid is not None) else ng
        sl = slice(q * ng, q * ng + nq)
        ratio(y[sl], yr[sl], yb[sl], tag + " y", rat)
        if train:
            ratio(sm[q], stats[q][0], 2 * U * stats[q][0].abs(), tag + " save_mean", rat)
            ratio(si[q], stats[q][1], 2 * U * stats[q][1], tag + " save_invstd", rat)
    assert not torch.isnan(y).any(), "NaN left in y (padding images are written too)"
    if train:
        ratio(rm, rmr, rmb, tag + " running_mean", rat)
        ratio(rv, rvr, rvb, tag + " running_var", rat)


def finish(rat):
    print("  ".join(f"{k}={v:.3f}" for k, v in rat.items()))
    for k, v in rat.items():
        assert v <= 1.0, f"{k}: {v:.3f} x its bound"


SHAPES = [(hw, ng, C, groups) for hw in (49, 9, 1) for ng in (2, 3) for C in (4, 8, 256) for groups in (1, 2)]


@pytest.mark.parametrize("hw,ng,C,groups", SHAPES)
def test_bn2d_edge_shapes(hw, ng, C, groups):
    """Train forward (+ LeakyReLU on the odd cases) and backward at rows per call that are no power of two; the
    reduction runs chunks of chan_chunk(ng hw) rows (grid = rows / R in the record).  chan_chunk halves 128 until it
    divides the rows of a call, so with an odd hw it ends at 2 rows for two images per call and at 1 row for three
    (never at 7: only powers of two are tried), which the record must show."""
    O = ops()
    n, act = ng * groups, (hw + ng + C // 4 + groups) % 2
    d = make(n, hw, C, seed=1000 * hw + 100 * ng + C + groups)
    rat = {}
    out = run_fwd(d, n, hw, C, groups, act)
    assert [l.kernel for l in out[5]] == ["cgl_chan_reduce4", "cgl_bn_finalize", "cgl_eltwise"]
    assert n * hw // out[5][0].grid == (2 if ng == 2 else 1), "rows per reduction chunk"
    ref = fwd_ref(d, n, hw, C, groups, act)
    check_fwd(out, ref, n, hw, C, groups, rat, "fwd")
    y, _, _, sm, si, _ = out
    slope32 = float(torch.tensor(SLOPE, dtype=torch.float32))
    dy64 = d["dy"].double()
    g64 = torch.where(y.cpu() > 0, dy64, dy64 * slope32) if act else dy64      # post = the y the op is given
    dx, dxbuf = padded(n * hw * C)
    dx.fill_(float("nan"))
    dg, dgbuf = padded(C)
    db, dbbuf = padded(C)
    O.bn2d_bwd(d["dy"].to(DEV), d["x"].to(DEV), n, hw, C, sm.contiguous(), si.contiguous(), d["gamma"].to(DEV), dx,
               groups=groups, post=y.contiguous() if act else None, dgamma=dg, dbeta=db, slope=SLOPE)
    assert kernels() == ["cgl_chan_reduce4", "cgl_bn_finalize", "cgl_eltwise"]
    torch.cuda.synchronize()
    for t, b, k in ((dx, dxbuf, "dx"), (dg, dgbuf, "dgamma"), (db, dbbuf, "dbeta")):
        canary_ok(b, t.numel(), k)
    dxr, dxb, (dgr, dgb), (dbr, dbb) = bwd_ref(d, n, hw, C, groups, lambda sl: g64[sl])
    ratio(dx.view(n, hw, C), dxr, dxb, "dX", rat)
    ratio(dg, dgr, dgb, "dgamma", rat)
    ratio(db, dbr, dbb, "dbeta", rat)
    finish(rat)


@pytest.mark.parametrize("hw,n,C,groups", [(49, 3, 8, 1), (9, 4, 256, 2), (1, 1, 4, 1)])
def test_bn2d_eval(hw, n, C, groups):
    d = make(n, hw, C, seed=hw + n + C)
    rat = {}
    out = run_fwd(d, n, hw, C, groups, act=1, train=False)
    assert [l.kernel for l in out[5]] == ["cgl_bn_finalize", "cgl_eltwise"]
    check_fwd(out, fwd_ref(d, n, hw, C, groups, 1, train=False), n, hw, C, groups, rat, "eval", train=False)
    assert torch.equal(out[1].cpu(), d["rm"]) and torch.equal(out[2].cpu(), d["rv"]), "eval wrote running statistics"
    finish(rat)


def _fwd_partials(x, n, hw, C, groups, R, valid):
    """{sum, M2 about the chunk mean} per R-row chunk in fp64, as a forward epilogue writes them: chunk q of the
    short first call holds min(max(valid hw - q R, 0), R) rows"""
    ng = n // groups
    rows = x.double().reshape(n * hw, C)
    part = torch.zeros(n * hw // R, C, 2, dtype=torch.float64)
    for ch in range(n * hw // R):
        r0, r1 = ch * R, (ch + 1) * R
        if r0 < ng * hw and valid is not None:
            r1 = max(r0, min(r1, valid * hw))
        if r1 > r0:
            blk = rows[r0:r1]
            part[ch, :, 0] = blk.sum(0)
            part[ch, :, 1] = ((blk - blk.mean(0)) ** 2).sum(0)
    return part


@pytest.mark.parametrize("scalar", [False, True], ids=["reduce4", "scalar"])
@pytest.mark.parametrize("nvk", ["one", "all-but-one", "all"])
@pytest.mark.parametrize("hw,ng,C,groups", [(49, 3, 8, 2), (9, 4, 256, 1), (16, 4, 64, 2)])
def test_bn2d_nvalid(hw, ng, C, groups, nvk, scalar):
    """The short real batch on cgl_bn2d_fwd, cgl_bn2d_fwd_stats(_coef), cgl_bn2d_bwd and cgl_bn2d_bwd_stats.  The
    _stats forms take partials restated here in fp64 (what a conv epilogue writes), so the finalize and the apply
    are held to the reference by themselves.
    What nvalid does in each: the forward reduction (mode 0) skips the padding rows, the forward finalize counts
    the valid rows only; in the backward nvalid reaches only the finalize's count and the apply's zeroing -- the
    mode 1 reduction sums every row, relying on the contract that padding images carry no loss and so a zero
    upstream gradient (set here: dy of the padding images is 0, as cgl_adv_loss's nvalid leaves it).  The backward
    cases therefore do not exercise a row limit in the reduction; there is none."""
    O = ops()
    n = ng * groups
    nv = {"one": 1, "all-but-one": ng - 1, "all": ng}[nvk]
    d = make(n, hw, C, seed=7 * hw + ng + C + groups + nv)
    d["dy"][nv:ng] = 0            # padding images carry no loss, so no gradient arrives (cgl_adv_loss's nvalid)
    rat = {}
    ref = fwd_ref(d, n, hw, C, groups, 1, valid=nv)
    out = run_fwd(d, n, hw, C, groups, 1, nv=nv, scalar=scalar)
    assert out[5][0].kernel == ("cgl_chan_reduce" if scalar else "cgl_chan_reduce4") and "NVALID" in out[5][0].flags
    assert "NVALID" in out[5][1].flags
    check_fwd(out, ref, n, hw, C, groups, rat, "fwd", valid=nv)
    # the same from epilogue partials: R = the largest power of two <= 32 that divides the rows of a call
    R = max(r for r in (1, 2, 4, 8, 16, 32) if (ng * hw) % r == 0)
    nvd = torch.tensor([nv], dtype=torch.int32, device=DEV)
    part = _fwd_partials(d["x"], n, hw, C, groups, R, nv).to(DEV)
    for coef in (False, True):
        y2, y2buf = padded(n * hw * C)
        rm, rv = d["rm"].to(DEV), d["rv"].to(DEV)
        sm, si = torch.empty(groups, C, device=DEV), torch.empty(groups, C, device=DEV)
        cf, cfbuf = padded(2 * groups * C)
        O.bn2d_fwd_stats(part, d["x"].to(DEV), n, hw, C, d["gamma"].to(DEV), d["beta"].to(DEV), y2, groups=groups,
                         eps=EPS, momentum=MOM, running_mean=rm, running_var=rv, act=1, slope=SLOPE, save_mean=sm,
                         save_invstd=si, R=R, coef=cf if coef else None, nvalid=nvd)
        ls = O.last_launches()
        assert [l.kernel for l in ls] == ["cgl_bn_finalize", "cgl_eltwise"] and "NVALID" in ls[0].flags
        torch.cuda.synchronize()
        canary_ok(y2buf, y2.numel(), "y (stats)")
        canary_ok(cfbuf, cf.numel(), "coef")
        check_fwd((y2.view(n, hw, C), rm, rv, sm, si, None), ref, n, hw, C, groups, rat,
                  "fwd_stats_coef" if coef else "fwd_stats", valid=nv)
    # backward: bn2d_bwd reduces, bn2d_bwd_stats takes {sum g, sum g (x - mean)} per chunk
    y, _, _, sm, si, _ = out
    slope32 = float(torch.tensor(SLOPE, dtype=torch.float32))
    dy64 = d["dy"].double()
    g64 = torch.where(y.cpu() > 0, dy64, dy64 * slope32)                       # post = the y the op is given
    dxr, dxb, (dgr, dgb), (dbr, dbb) = bwd_ref(d, n, hw, C, groups, lambda sl: g64[sl], valid=nv)
    gsm = sm.cpu().double()
    bpart = torch.zeros(n * hw // R, C, 2, dtype=torch.float64)
    grow, xrow = g64.reshape(n * hw, C), d["x"].double().reshape(n * hw, C)
    for ch in range(n * hw // R):
        blk = slice(ch * R, (ch + 1) * R)
        bpart[ch, :, 0] = grow[blk].sum(0)
        bpart[ch, :, 1] = (grow[blk] * (xrow[blk] - gsm[ch * R // (ng * hw)])).sum(0)
    for stats in (False, True):
        dx, dxbuf = padded(n * hw * C)
        dx.fill_(float("nan"))
        dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        args = (d["dy"].to(DEV), d["x"].to(DEV), n, hw, C, sm.contiguous(), si.contiguous(), d["gamma"].to(DEV), dx)
        kw = dict(groups=groups, post=y.contiguous(), dgamma=dg, dbeta=db, slope=SLOPE, nvalid=nvd)
        with scalar_reduce(scalar):
            if stats:
                O.bn2d_bwd_stats(bpart.to(DEV), *args, R=R, **kw)
            else:
                O.bn2d_bwd(*args, **kw)
            ls = O.last_launches()
        want = ["cgl_bn_finalize", "cgl_eltwise"]
        assert [l.kernel for l in ls] == (want if stats else ["cgl_chan_reduce" if scalar else "cgl_chan_reduce4"] + want)
        assert "NVALID" in ls[-1].flags and "NVALID" in ls[-2].flags
        torch.cuda.synchronize()
        canary_ok(dxbuf, dx.numel(), "dx")
        tag = "bwd_stats" if stats else "bwd"
        dxv = dx.view(n, hw, C)
        assert bool((dxv[nv:ng] == 0).all()), "padding images must get a zero input gradient"
        ratio(dxv, dxr, dxb, tag + " dX", rat)
        ratio(dg, dgr, dgb, tag + " dgamma", rat)
        ratio(db, dbr, dbb, tag + " dbeta", rat)
    finish(rat)


def chan_chunk(gr):
    """chan_chunk's default rule (csrc/cgl_conv_bn.h, CGL_CHAN_MINCH unset): the rows per chunk of cgl_bn2d_fwd's and
    cgl_bn2d_bwd's own reduction"""
    R = 128
    while R > 1 and gr % R:
        R //= 2
    while R > 32 and gr // R < 64 and gr % (R // 2) == 0:
        R //= 2
    return R


def own_partials(n, hw, C, groups, R):
    """The chunk partials [n hw / R][C][2] (double) that cgl_bn2d_fwd / cgl_bn2d_bwd left at the start of the
    stream's workspace, cloned: the next call carves its coefficients out of the same buffer."""
    O = ops()
    ws = O.workspace(O.bn2d_ws_bytes(n, hw, C, groups), DEV)
    return ws[:n * hw // R * C * 16].view(torch.float64).clone()


# (hw, images per call, C, groups, nvalid): 147 rows per call (odd: chunks of one row), 64 rows per call in two
# chunks of 32, and the latter as a short first call
ONE_PATH = [(49, 3, 8, 2, None), (16, 4, 64, 2, None), (16, 4, 64, 2, 1)]


def _one_path_setup(hw, ng, groups):
    if "CGL_CHAN_MINCH" in os.environ:
        pytest.skip("chan_chunk is restated here for the default CGL_CHAN_MINCH")
    return ops(), ng * groups, chan_chunk(ng * hw)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("hw,ng,C,groups,nv", ONE_PATH)
def test_bn2d_fwd_entry_points_are_one_path(hw, ng, C, groups, nv, act):
    """cgl_bn2d_fwd is its own channel reduction followed by what cgl_bn2d_fwd_stats does: given the partials the
    first left in the workspace and its chunk size, the second must write the same bits (y, saved and running
    statistics) from the same launches less the reduction -- the unsliced finalize, as no scratch is given."""
    O, n, R = _one_path_setup(hw, ng, groups)
    d = make(n, hw, C, seed=11 * hw + ng + C + groups + act)
    y, rm, rv, sm, si, ls = run_fwd(d, n, hw, C, groups, act, nv=nv)
    part = own_partials(n, hw, C, groups, R)
    assert [l.kernel for l in ls] == ["cgl_chan_reduce4", "cgl_bn_finalize", "cgl_eltwise"]
    assert ls[0].grid == n * hw // R, "rows per reduction chunk"
    y2, y2buf = padded(n * hw * C)
    y2.fill_(float("nan"))
    rm2, rv2 = d["rm"].to(DEV), d["rv"].to(DEV)
    sm2, si2 = torch.empty(groups, C, device=DEV), torch.empty(groups, C, device=DEV)
    nvd = torch.tensor([nv], dtype=torch.int32, device=DEV) if nv is not None else None
    O.bn2d_fwd_stats(part, d["x"].to(DEV), n, hw, C, d["gamma"].to(DEV), d["beta"].to(DEV), y2, groups=groups, eps=EPS,
                     momentum=MOM, running_mean=rm2, running_var=rv2, act=act, slope=SLOPE, save_mean=sm2,
                     save_invstd=si2, R=R, nvalid=nvd)
    assert O.last_launches() == ls[1:], "the record of cgl_bn2d_fwd less its reduction"
    torch.cuda.synchronize()
    canary_ok(y2buf, y2.numel(), "y (stats)")
    assert not torch.isnan(y).any(), "NaN left in y"
    for a, b, k in ((y, y2.view(n, hw, C), "y"), (sm, sm2, "save_mean"), (si, si2, "save_invstd"),
                    (rm, rm2, "running_mean"), (rv, rv2, "running_var")):
        assert torch.equal(a, b), f"{k}: cgl_bn2d_fwd and cgl_bn2d_fwd_stats differ"


@pytest.mark.parametrize("hw,ng,C,groups,nv,how", [s + ("post",) for s in ONE_PATH] + [(16, 8, 64, 1, None, "post_coef")])
def test_bn2d_bwd_entry_points_are_one_path(hw, ng, C, groups, nv, how):
    """cgl_bn2d_bwd against cgl_bn2d_bwd_stats on the partials it left: dX, dgamma and dbeta to the bit, and the
    same launches less the reduction.  LeakyReLU' from post, and once from post_coef (one call: groups = 1)."""
    O, n, R = _one_path_setup(hw, ng, groups)
    d = make(n, hw, C, seed=13 * hw + ng + C + groups)
    if nv is not None:
        d["dy"][nv:ng] = 0            # padding images carry no loss (test_bn2d_nvalid)
    y, _, _, sm, si, _ = run_fwd(d, n, hw, C, groups, 1, nv=nv)
    if how == "post":
        kw = dict(post=y.contiguous())
    else:
        g = torch.Generator().manual_seed(5)
        coef = torch.stack([torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)]).float().contiguous()
        kw = dict(post_coef=(coef.to(DEV), 0, 1))
    nvd = torch.tensor([nv], dtype=torch.int32, device=DEV) if nv is not None else None
    kw.update(groups=groups, slope=SLOPE, nvalid=nvd)
    res, part, ls1 = [], None, None
    for stats in (False, True):
        dx, dxbuf = padded(n * hw * C)
        dx.fill_(float("nan"))
        dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        args = (d["dy"].to(DEV), d["x"].to(DEV), n, hw, C, sm.contiguous(), si.contiguous(), d["gamma"].to(DEV), dx)
        if stats:
            O.bn2d_bwd_stats(part, *args, R=R, dgamma=dg, dbeta=db, **kw)
            assert O.last_launches() == ls1[1:], "the record of cgl_bn2d_bwd less its reduction"
        else:
            O.bn2d_bwd(*args, dgamma=dg, dbeta=db, **kw)
            ls1 = O.last_launches()
            part = own_partials(n, hw, C, groups, R)
            assert [l.kernel for l in ls1] == ["cgl_chan_reduce4", "cgl_bn_finalize", "cgl_eltwise"]
            assert ls1[0].grid == n * hw // R, "rows per reduction chunk"
        torch.cuda.synchronize()
        canary_ok(dxbuf, dx.numel(), "dx")
        res.append((dx, dg, db))
    for a, b, k in zip(res[0], res[1], ("dX", "dgamma", "dbeta")):
        assert not torch.isnan(a).any() and torch.equal(a, b), f"{k}: cgl_bn2d_bwd and cgl_bn2d_bwd_stats differ"


@pytest.mark.parametrize("ints", [False, True], ids=["normal", "integers"])
@pytest.mark.parametrize("mode", ["post", "post_coef", "neither"])
def test_chan_reduce_scalar_bwd(mode, ints):
    """Mode 1 of the 4-byte reduction (CGL_CHAN_SCALAR=1) with post, with post_coef and with neither, against fp64
    and against cgl_chan_reduce4 on the same inputs.  With post_coef the 4-byte kernel once took LeakyReLU'
    from fmaf(xv[i], ...) BEFORE loading xv[i]: the sign came from a stale register.  On integer data sum g and
    sum g (x - mean) are exact in both kernels, so dbeta must equal the fp64 sum and the two kernels must agree
    bit for bit."""
    O = ops()
    n, hw, C = 3, 49, 8
    d = make(n, hw, C, seed=len(mode) + 17, ints=ints)
    g = torch.Generator().manual_seed(5)
    if ints:
        coef = torch.stack([torch.tensor([0.5, 1.0, 2.0, -1.0])[torch.randint(0, 4, (C,), generator=g)],
                            torch.randint(-1, 2, (C,), generator=g).float() + 0.5]).contiguous()
        mean = torch.randint(-1, 2, (1, C), generator=g).float()
    else:
        coef = torch.stack([torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)]).float().contiguous()
        mean = d["x"].double().reshape(-1, C).mean(0).float().view(1, C)
    invstd = (1.0 / torch.sqrt(d["x"].double().reshape(-1, C).var(0, unbiased=False) + EPS)).float().view(1, C)
    slope = 0.25 if ints else SLOPE
    slope32 = float(torch.tensor(slope, dtype=torch.float32))
    x64, dy64 = d["x"].double(), d["dy"].double()
    pre = x64 * coef[0].double() + coef[1].double()            # the forward's fmaf(x, scale, shift)
    post = torch.where(pre > 0, pre, pre * slope32).float()
    g64 = dy64 if mode == "neither" else torch.where(pre > 0, dy64, dy64 * slope32)
    # the op's own inputs: save_mean / save_invstd as given (fp32)
    m64, i64, gam = mean.double()[0], invstd.double()[0], d["gamma"].double()
    rows = n * hw
    xc = x64.reshape(rows, C) - m64
    gr = g64.reshape(rows, C)
    S, D = gr.sum(0), (xc * gr).sum(0)
    t2, t3 = S / rows, xc * D * i64 * i64 / rows
    dxr = ((gr - t2 - t3) * i64 * gam).reshape(n, hw, C)
    dxb = (16 * U * (gr.abs() + t2.abs() + t3.abs()) * i64 * gam.abs()).reshape(n, hw, C)
    res = {}
    rat = {}
    for scalar in (True, False):
        dx, dxbuf = padded(n * hw * C)
        dx.fill_(float("nan"))
        dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        kw = dict(post=post.to(DEV)) if mode == "post" else (dict(post_coef=(coef.to(DEV), 0, 1)) if mode == "post_coef"
                                                             else {})
        with scalar_reduce(scalar):
            O.bn2d_bwd(d["dy"].to(DEV), d["x"].to(DEV), n, hw, C, mean.to(DEV), invstd.to(DEV), d["gamma"].to(DEV), dx,
                       dgamma=dg, dbeta=db, slope=slope, **kw)
            ls = O.last_launches()
        assert ls[0].kernel == ("cgl_chan_reduce" if scalar else "cgl_chan_reduce4") and ls[0].tm == 1
        torch.cuda.synchronize()
        canary_ok(dxbuf, dx.numel(), "dx")
        tag = "scalar" if scalar else "reduce4"
        ratio(dx.view(n, hw, C), dxr, dxb, tag + " dX", rat)
        ratio(dg, D * i64, 8 * U * i64 * (xc * gr).abs().sum(0), tag + " dgamma", rat)
        ratio(db, S, 8 * U * gr.abs().sum(0), tag + " dbeta", rat)
        if ints:
            assert torch.equal(db.cpu().double(), S), f"{tag}: dbeta is not the exact sum"
        res[scalar] = (dx.clone(), dg.clone(), db.clone())
    if ints:
        for a, b, k in zip(res[True], res[False], ("dX", "dgamma", "dbeta")):
            assert torch.equal(a, b), f"{k}: the 4-byte and the 16-byte reduction differ on exact sums"
    finish(rat)


@pytest.mark.parametrize("nv", [None, 2])
def test_chan_reduce_scalar_fwd(nv):
    """Mode 0 of the 4-byte reduction with and without nvalid (C = 8, 49-pixel maps: chunks of one row)."""
    n, hw, C, groups = 6, 49, 8, 2
    d = make(n, hw, C, seed=31)
    rat = {}
    ref = fwd_ref(d, n, hw, C, groups, 0, valid=nv)
    for scalar in (True, False):
        out = run_fwd(d, n, hw, C, groups, 0, nv=nv, scalar=scalar)
        assert out[5][0].kernel == ("cgl_chan_reduce" if scalar else "cgl_chan_reduce4") and out[5][0].tm == 0
        check_fwd(out, ref, n, hw, C, groups, rat, "scalar" if scalar else "reduce4", valid=nv)
    finish(rat)


# (n, h, w, cin, cout, the kernel of the column-sum pass): weight gradients whose bias gradient is a column sum of dY
# -- >= 2^28 MACs and K % 64 == 0, so the MFMA kernel carries no bias column
COLSUM = [
    (228, 32, 32, 64, 2, "cgl_chan_reduce", False),          # C = 2: the 4-byte form is the only one
    (8, 32, 32, 64, 64, "cgl_chan_reduce", True),            # mode 2 of the 4-byte form at C % 4 == 0 (CGL_CHAN_SCALAR)
    (8, 32, 32, 64, 64, "cgl_chan_reduce4", False),
    (5, 31, 33, 64, 96, "cgl_colsum_k", False),              # C no power of two, 5115 rows: a last chunk of 27
]


@pytest.mark.parametrize("n,h,w,cin,cout,kernel,scalar", COLSUM)
def test_bias_column_sums(n, h, w, cin, cout, kernel, scalar):
    """db of cgl_conv3x3_bwd_weight by column sums (mode 2 reductions, cgl_colsum_k) against the fp64 column sums
    of dY: exact on integer data (double partials of whole numbers), within 8 u sum |dy| on normal data.  (C = 1
    runs in test_gpu_conv_routes.py's one-output-channel weight gradients.)  dW is checked there, not here."""
    O = ops()
    g = torch.Generator(device=DEV).manual_seed(n + cout)
    x = torch.randn(n, h, w, cin, device=DEV, generator=g)
    dw = torch.empty(cout, cin, 3, 3, device=DEV)
    rat = {}
    for ints in (True, False):
        dy = (torch.randint(-2, 3, (n, h, w, cout), device=DEV, generator=g).float() if ints
              else torch.randn(n, h, w, cout, device=DEV, generator=g))
        db, dbbuf = padded(cout)
        db.fill_(float("nan"))
        with scalar_reduce(scalar):
            O.conv3x3_bwd_weight(dy, x, dw, db, n, h, w, cin, cout)
            ls = O.last_launches()
        assert [l.kernel for l in ls][-2:] == [kernel, "cgl_bn_finalize"], [l.kernel for l in ls]
        assert ls[-2].tm == (0 if kernel == "cgl_colsum_k" else 2) and ls[-1].tm == 2
        torch.cuda.synchronize()
        canary_ok(dbbuf, cout, "db")
        d64 = dy.double().reshape(-1, cout)
        ref = d64.sum(0).cpu()
        if ints:
            assert torch.equal(db.cpu().double(), ref)
        else:
            ratio(db, ref, 8 * U * d64.abs().sum(0).cpu(), "db", rat)
    finish(rat)


def test_bn2d_bwd_stats_colsum_part():
    """colsum_part of cgl_bn2d_bwd_stats (cgl_bnb_apply_colsum): per 256-row chunk the column sums of the dX it
    stores, {sum, 0} -- held against the fp64 sums of that dX (double accumulation of 256 fp32 values: 2^-44
    relative to sum |dX| is generous), and dX itself against the reference."""
    O = ops()
    n, hw, C, R = 4, 128, 8, 32
    d = make(n, hw, C, seed=77)
    out = run_fwd(d, n, hw, C, 1, 0)
    sm, si = out[3], out[4]
    g64, x64 = d["dy"].double().reshape(-1, C), d["x"].double().reshape(-1, C)
    bpart = torch.zeros(n * hw // R, C, 2, dtype=torch.float64)
    for ch in range(n * hw // R):
        blk = slice(ch * R, (ch + 1) * R)
        bpart[ch, :, 0] = g64[blk].sum(0)
        bpart[ch, :, 1] = (g64[blk] * (x64[blk] - sm.cpu().double()[0])).sum(0)
    dx, dxbuf = padded(n * hw * C)
    cs, csbuf = padded(n * hw // 256 * C * 2, torch.float64)
    O.bn2d_bwd_stats(bpart.to(DEV), d["dy"].to(DEV), d["x"].to(DEV), n, hw, C, sm.contiguous(), si.contiguous(),
                     d["gamma"].to(DEV), dx, R=R, colsum=cs, slope=SLOPE)
    assert kernels() == ["cgl_bn_finalize", "cgl_bnb_apply_colsum"]
    torch.cuda.synchronize()
    canary_ok(dxbuf, dx.numel(), "dx")
    canary_ok(csbuf, cs.numel(), "colsum_part")
    rat = {}
    dxr, dxb, _, _ = bwd_ref(d, n, hw, C, 1, lambda sl: d["dy"].double()[sl])
    ratio(dx.view(n, hw, C), dxr, dxb, "dX", rat)
    chunks = dx.double().view(n * hw // 256, 256, C)
    csv = cs.view(n * hw // 256, C, 2)
    assert bool((csv[:, :, 1] == 0).all())
    ratio(csv[:, :, 0], chunks.sum(1).cpu(), 2.0 ** -44 * chunks.abs().sum(1).cpu(), "colsum_part", rat)
    finish(rat)


def test_eltwise_grid_wrap():
    """One forward and one backward with n hw C just above 4 * 8192 * 256 floats, so cgl_eltwise's 8192-block grid
    wraps: the 8 rows past the wrap are checked by themselves."""
    O = ops()
    n, hw, C = 2, 65540, 64
    wrap_row = 4 * 8192 * 256 // C
    assert n * hw > wrap_row
    d = make(n, hw, C, seed=3)
    rat = {}
    out = run_fwd(d, n, hw, C, 1, 1)
    assert out[5][-1].kernel == "cgl_eltwise" and out[5][-1].grid == 8192
    ref = fwd_ref(d, n, hw, C, 1, 1)
    check_fwd(out, ref, n, hw, C, 1, rat, "fwd")
    y, _, _, sm, si, _ = out
    ratio(y.reshape(-1, C)[wrap_row:], ref[1].reshape(-1, C)[wrap_row:], ref[2].reshape(-1, C)[wrap_row:],
          "fwd y past the wrap", rat)
    slope32 = float(torch.tensor(SLOPE, dtype=torch.float32))
    dy64 = d["dy"].double()
    g64 = torch.where(y.cpu() > 0, dy64, dy64 * slope32)
    dx, dxbuf = padded(n * hw * C)
    dx.fill_(float("nan"))
    dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    O.bn2d_bwd(d["dy"].to(DEV), d["x"].to(DEV), n, hw, C, sm.contiguous(), si.contiguous(), d["gamma"].to(DEV), dx,
               post=y.contiguous(), dgamma=dg, dbeta=db, slope=SLOPE)
    ls = O.last_launches()
    assert ls[-1].kernel == "cgl_eltwise" and ls[-1].grid == 8192
    torch.cuda.synchronize()
    canary_ok(dxbuf, dx.numel(), "dx")
    dxr, dxb, (dgr, dgb), (dbr, dbb) = bwd_ref(d, n, hw, C, 1, lambda sl: g64[sl])
    ratio(dx.view(n, hw, C), dxr, dxb, "dX", rat)
    ratio(dx.view(-1, C)[wrap_row:], dxr.reshape(-1, C)[wrap_row:], dxb.reshape(-1, C)[wrap_row:], "dX past the wrap",
          rat)
    ratio(dg, dgr, dgb, "dgamma", rat)
    ratio(db, dbr, dbb, "dbeta", rat)
    finish(rat)
