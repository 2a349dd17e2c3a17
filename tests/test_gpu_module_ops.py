"""The single ops under the drop-in nn.Module API (cglgan.model): BatchNorm1d forward / backward
(cgl_bn1d_fwd -> cgl_bn1d_fwd_k, cgl_bn1d_bwd -> cgl_bn_bwd_arg = cgl_bn_bwd_body<32>) and the elementwise
activations (cgl_act_fwd / cgl_act_bwd), each against a plain fp64 reference computed on the CPU from the
same fp32 inputs the kernel got.

The shapes reach both code paths of the BatchNorm kernels (rows in registers for M <= 256, streamed twice
above), the ragged last 32-feature block, ldx > F (pad columns hold NaN), M = 2 and M = 1 (eval), and the
wrapped grid-stride loop of the activations (n > 4096 * 256).

Bounds, u = 2^-24 (derivations: DESIGN.md section 5, "Op-level bounds"; the kernel accumulates the column
sums in double, so only the final fp32 roundings count):
  save_mean 1 ulp, save_invstd 2 ulp, running_mean / running_var 2 ulp of the fp64 value;
  y:  |y - y64| <= 16 u (|x sc| + |beta| + |mean sc| + |y64|),  sc = invstd gamma  (y = fma(x, sc32, sh32) with
      sc32 = fp32(invstd) gamma and sh32 = beta - mean sc32, each rounded: the error of sh32 is ~2 u |mean sc| + u |sh|
      and does not shrink when beta - mean sc cancels.  A first form of this bound had |sh| in place of
      |beta| + |mean sc|; eval mode with running_mean ~ N(0, 1) met a column with beta = -0.29277, mean sc = -0.29223
      and x ~ 0, where the kernel is 5.1x over that form -- reproduced exactly by a numpy emulation of the rounding
      sequence -- and 0.01x of this one);
  dX: |dX - ref| <= 16 u (|dy| + |S / M| + |(x - mean) D invstd^2 / M|) invstd |gamma|;
  dgamma: 8 u invstd sum |(x - mean) dy|;  dbeta: 8 u sum |dy|.
Each test prints its worst ratio to the bound.  Measured on the MI355X (worst |err| / bound over the cases):
  bn1d_fwd train: save_mean 0.50 (of 1 ulp: correctly rounded), save_invstd 0.25, y 0.07, running_mean 0.25,
  running_var 0.25;  eval: y 0.09;  bn1d_bwd: dX 0.25, dgamma 0.06, dbeta 0.10;
  act_fwd: Tanh equal to the correctly rounded fp32 tanh at every value (0 of 1 048 579 differ), Sigmoid 0.31;
  act_bwd: Tanh 0.50 ulp, Sigmoid 0.49.
"""
import ctypes

import numpy as np
import pytest
import torch

from parity_helpers import KINK_MARGIN

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SLOPE = 0.2
E_ARG = -1


def _C():
    from cglgan import _lib as C
    return C


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _ws():
    return torch.zeros(_C().lib.cgl_op_workspace_bytes(), dtype=torch.uint8, device="cuda")


def _ulp32(x):
    """fp32 spacing at |x| (x: float64 tensor)"""
    return torch.from_numpy(np.spacing(np.abs(x.numpy()).astype(np.float32)).astype(np.float64))


# (M, F, ldx): smallest legal | ragged F, registers | last register-path M, ldx > F | first streamed M |
# streamed, M % 8 != 0, one partial block | streamed, two feature blocks
BN_CASES = [(2, 1, 1), (37, 33, 33), (256, 40, 48), (257, 40, 40), (1000, 7, 12), (300, 64, 64)]
EPS, MOM = 0.8, 0.1     # the reference's BatchNorm1d(out, 0.8)


def _bn_inputs(M, F, act, seed0, mean=0.0, std=1.0, eps=EPS, stats=None):
    """fp32 inputs (CPU) and the fp64 forward reference.  act == 1: the seed is the first from seed0 whose
    pre-activations all lie at least KINK_MARGIN std from 0 (chosen from the fp64 reference alone).
    stats = (running_mean, running_var): eval mode."""
    for seed in range(seed0, seed0 + 64):
        g = torch.Generator().manual_seed(seed)
        x = (mean + std * torch.randn(M, F, generator=g)).float()
        gamma = (0.5 + torch.rand(F, generator=g)) * torch.where(torch.rand(F, generator=g) < 0.3, -1.0, 1.0)
        beta = torch.randn(F, generator=g)
        x64 = x.double()
        if stats is None:
            m64 = x64.mean(0)
            q64 = ((x64 - m64) ** 2).sum(0)
            var = q64 / M
        else:
            m64, var, q64 = stats[0].double(), stats[1].double(), None
        inv64 = 1.0 / torch.sqrt(var + eps)
        sc = inv64 * gamma.double()
        sh = beta.double() - m64 * sc
        pre = x64 * sc + sh
        if act == 0 or float(pre.abs().min()) >= KINK_MARGIN * float(pre.std() if pre.numel() > 1 else 1.0):
            break
    else:
        raise RuntimeError("no well-conditioned seed found")
    y64 = torch.where(pre > 0, pre, pre * float(np.float32(SLOPE))) if act else pre
    # (|beta| + |mean sc|, not |sh|: the kernel forms sh = beta - mean sc32 with the ROUNDED sc32 = fp32(invstd) gamma,
    # so sh carries ~2 u |mean sc| whatever is left after the subtraction cancels)
    ybound = 16 * U * ((x64 * sc).abs() + beta.double().abs() + (m64 * sc).abs() + y64.abs())
    return dict(x=x, gamma=gamma.float(), beta=beta.float(), mean=m64, q=q64, invstd=inv64, y=y64, ybound=ybound)


def _padded(x, ldx):
    """x [M, F] in a device buffer of row stride ldx whose pad columns hold NaN"""
    M, F = x.shape
    buf = torch.full((M, ldx), float("nan"), device="cuda")
    buf[:, :F] = x.cuda()
    return buf


def _bn_fwd(X, M, F, ldx, gamma, beta, eps, rm, rv, train, act, save=True, rc_only=False):
    C = _C()
    Y = torch.full((M * F + 8,), -7.0, device="cuda")      # 8 sentinel words past the output
    sm = torch.full((F + 4,), -7.0, device="cuda") if save else None
    si = torch.full((F + 4,), -7.0, device="cuda") if save else None
    ws = _ws()
    rc = C.lib.cgl_bn1d_fwd(_p(X), M, F, ldx, _p(gamma), _p(beta), eps, MOM, _p(rm), _p(rv), train, act, SLOPE, _p(Y),
                            _p(sm), _p(si), _p(ws), ws.numel(), _s())
    if rc_only:
        return rc
    C.check(rc, "cgl_bn1d_fwd")
    torch.cuda.synchronize()
    assert (Y[M * F:] == -7.0).all(), "stores past Y"
    if save:
        assert (sm[F:] == -7.0).all() and (si[F:] == -7.0).all(), "stores past save_mean / save_invstd"
        return Y[:M * F].view(M, F), sm[:F], si[:F]
    return Y[:M * F].view(M, F), None, None


def _ratio(got, ref, bound):
    err = (got.double().cpu() - ref).abs()
    assert torch.isfinite(got).all()
    return float((err / bound.clamp_min(1e-300)).max())


def _check_train(M, F, ldx, act, mean=0.0, std=1.0, eps=EPS):
    r = _bn_inputs(M, F, act, seed0=1000 * M + F + act, mean=mean, std=std, eps=eps)
    X = _padded(r["x"], ldx)
    g = torch.Generator().manual_seed(5)
    rm0 = torch.randn(F, generator=g)
    rv0 = 0.5 + torch.rand(F, generator=g)
    rm, rv = rm0.cuda(), rv0.cuda()
    Y, sm, si = _bn_fwd(X, M, F, ldx, r["gamma"].cuda(), r["beta"].cuda(), eps, rm, rv, 1, act)
    rat = {
        "mean": _ratio(sm, r["mean"], _ulp32(r["mean"])),
        "invstd": _ratio(si, r["invstd"], 2 * _ulp32(r["invstd"])),
        "y": _ratio(Y, r["y"], r["ybound"]),
    }
    rm64 = MOM * r["mean"] + (1 - MOM) * rm0.double()
    rv64 = MOM * r["q"] / (M - 1) + (1 - MOM) * rv0.double()       # unbiased: Q / (M - 1)
    rat["run_mean"] = _ratio(rm, rm64, 2 * _ulp32(rm64))
    rat["run_var"] = _ratio(rv, rv64, 2 * _ulp32(rv64))
    print(f"bn1d_fwd train M={M} F={F} ldx={ldx} act={act} eps={eps}: worst ratio to bound "
          + " ".join(f"{k}={v:.3f}" for k, v in rat.items()))
    for k, v in rat.items():
        assert v <= 1.0, f"{k}: {v:.3f} x its bound"
    # running_* = NULL and save_* = NULL: the same y, bit for bit
    Y2, _, _ = _bn_fwd(X, M, F, ldx, r["gamma"].cuda(), r["beta"].cuda(), eps, None, None, 1, act, save=False)
    assert torch.equal(Y2, Y)
    return rat


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("M,F,ldx", BN_CASES)
def test_bn1d_fwd_train(M, F, ldx, act):
    """Worst ratios to the bounds on the MI355X: mean 0.50, invstd 0.25, y 0.07, running_mean / _var 0.25."""
    _check_train(M, F, ldx, act)


def test_bn1d_fwd_unbiased_variance_m2():
    """M = 2: running_var takes Q / (M - 1) = Q, twice the biased variance that the output uses."""
    F = 5
    x = torch.tensor([[1.0, -2.0, 0.5, 3.0, 10.0], [2.0, 2.0, 0.25, -3.0, 10.5]])
    rm, rv = torch.zeros(F, device="cuda"), torch.zeros(F, device="cuda")
    ones, zeros = torch.ones(F, device="cuda"), torch.zeros(F, device="cuda")
    _bn_fwd(x.cuda(), 2, F, F, ones, zeros, EPS, rm, rv, 1, 0)
    d = (x[0] - x[1]).double()
    q = d * d / 2                                                   # sum of squared deviations of two values
    want = MOM * q
    assert _ratio(rv, want, 2 * _ulp32(want)) <= 1.0
    assert float((rv.cpu().double() - MOM * q / 2).abs().min()) > 1e-3   # not the biased variance


@pytest.mark.parametrize("M", [64, 300])
def test_bn1d_fwd_train_large_mean_small_spread(M):
    """eps = 1e-5, columns of mean 100 and standard deviation 0.01: var ~ 1e-4 is 8 orders below mean^2, which a
    one-pass E[x^2] - E[x]^2 in fp32 (and barely in fp64) cannot resolve; the two-pass form must hold 2 ulp."""
    _check_train(M, 33, 33, 0, mean=100.0, std=0.01, eps=1e-5)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("M,F,ldx", BN_CASES + [(1, 33, 40)])
def test_bn1d_fwd_eval(M, F, ldx, act):
    """Worst ratio to the y bound on the MI355X: 0.09 (5.1 against the first form of the bound, see the module
    docstring: the case M = 257, act = 0)."""
    g = torch.Generator().manual_seed(77 + M)
    rm0 = torch.randn(F, generator=g)
    rv0 = 0.05 + 2 * torch.rand(F, generator=g)
    r = _bn_inputs(M, F, act, seed0=2000 * M + F + act, stats=(rm0, rv0))
    X = _padded(r["x"], ldx)
    rm, rv = rm0.cuda(), rv0.cuda()
    Y, _, _ = _bn_fwd(X, M, F, ldx, r["gamma"].cuda(), r["beta"].cuda(), EPS, rm, rv, 0, act, save=False)
    rat = _ratio(Y, r["y"], r["ybound"])
    print(f"bn1d_fwd eval M={M} F={F} ldx={ldx} act={act}: worst ratio to bound y={rat:.3f}")
    assert rat <= 1.0
    assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0), "eval mode changed the running statistics"


def _bn_bwd(dY, Y, X, M, F, sm, si, gamma, act, want_gb=True, ws=None):
    dX = torch.full((M * F + 8,), -7.0, device="cuda")
    dg = torch.full((F + 4,), -7.0, device="cuda") if want_gb else None
    db = torch.full((F + 4,), -7.0, device="cuda") if want_gb else None
    ws = _ws() if ws is None else ws
    return _bn_bwd_call(dict(dY=dY, Y=Y, X=X, sm=sm, si=si, gamma=gamma, dX=dX, dg=dg, db=db, ws=ws, wsb=ws.numel(),
                             M=M, F=F, act=act))


def _bn_bwd_call(a, rc_only=False):
    C = _C()
    M, F, dX, dg, db = a["M"], a["F"], a["dX"], a["dg"], a["db"]
    rc = C.lib.cgl_bn1d_bwd(_p(a["dY"]), _p(a["Y"]), _p(a["X"]), a["M"], a["F"], _p(a["sm"]), _p(a["si"]),
                            _p(a["gamma"]), a["act"], SLOPE, _p(a["dX"]), _p(a["dg"]), _p(a["db"]),
                            ctypes.c_void_p(a["wsp"]) if "wsp" in a else _p(a["ws"]), a["wsb"], _s())
    if rc_only:
        return rc
    C.check(rc, "cgl_bn1d_bwd")
    torch.cuda.synchronize()
    assert (dX[M * F:] == -7.0).all(), "stores past dX"
    if dg is not None:
        assert (dg[F:] == -7.0).all() and (db[F:] == -7.0).all(), "stores past dgamma / dbeta"
        return dX[:M * F].view(M, F), dg[:F], db[:F]
    return dX[:M * F].view(M, F), None, None


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("M,F,ldx", BN_CASES)
def test_bn1d_bwd(M, F, ldx, act):
    """Worst ratios to the bounds on the MI355X: dX 0.25, dgamma 0.06, dbeta 0.10."""
    r = _bn_inputs(M, F, act, seed0=3000 * M + F + act)
    X = r["x"].cuda()
    gamma = r["gamma"].cuda()
    Y, sm, si = _bn_fwd(X, M, F, F, gamma, r["beta"].cuda(), EPS, None, None, 1, act)
    dYc = torch.randn(M, F, generator=torch.Generator().manual_seed(M + F))
    dY = dYc.cuda()
    dX, dg, db = _bn_bwd(dY, Y if act else None, X, M, F, sm, si, gamma, act)
    # fp64 reference from the fp32 arrays the kernel read (its own save_mean / save_invstd and Y)
    x64, mean, inv, gm = r["x"].double(), sm.cpu().double(), si.cpu().double(), r["gamma"].double()
    dy = dYc.double()
    if act:
        dy = torch.where(Y.cpu() > 0, dy, dy * float(np.float32(SLOPE)))
    xc = x64 - mean
    S, D = dy.sum(0), (xc * dy).sum(0)
    t2, t3 = S / M, xc * D * inv * inv / M
    ref = (dy - t2 - t3) * inv * gm
    bound = 16 * U * (dy.abs() + t2.abs() + t3.abs()) * inv * gm.abs()
    rat = {
        "dX": _ratio(dX, ref, bound),
        "dgamma": _ratio(dg, D * inv, 8 * U * inv * (xc * dy).abs().sum(0)),
        "dbeta": _ratio(db, S, 8 * U * dy.abs().sum(0)),
    }
    print(f"bn1d_bwd M={M} F={F} act={act}: worst ratio to bound " + " ".join(f"{k}={v:.3f}" for k, v in rat.items()))
    for k, v in rat.items():
        assert v <= 1.0, f"{k}: {v:.3f} x its bound"
    # dgamma = dbeta = NULL: both land in the workspace, dX is the same bit for bit
    ws = _ws()
    dX2, _, _ = _bn_bwd(dY, Y if act else None, X, M, F, sm, si, gamma, act, want_gb=False, ws=ws)
    assert torch.equal(dX2, dX)
    scratch = ws.view(torch.float32)
    assert torch.equal(scratch[:F], dg) and torch.equal(scratch[F:2 * F], db)


def test_bn1d_bad_arguments():
    """Every CGL_E_ARG branch of cgl_bn1d_fwd and cgl_bn1d_bwd, one call each; nothing is launched."""
    M, F = 4, 3
    t = lambda *s: torch.zeros(*s, device="cuda")
    X, gamma, beta, rm, rv = t(M, F), t(F), t(F), t(F), t(F) + 1

    def fwd(**o):
        a = dict(X=X, M=M, F=F, ldx=F, gamma=gamma, beta=beta, rm=rm, rv=rv, train=1, act=0, Y=t(M, F), sm=t(F),
                 si=t(F))
        a.update(o)
        ws = _ws()
        return _C().lib.cgl_bn1d_fwd(_p(a["X"]), a["M"], a["F"], a["ldx"], _p(a["gamma"]), _p(a["beta"]), EPS, MOM,
                                     _p(a["rm"]), _p(a["rv"]), a["train"], a["act"], SLOPE, _p(a["Y"]), _p(a["sm"]),
                                     _p(a["si"]), _p(ws), ws.numel(), _s())

    assert fwd() == 0
    for bad in (dict(X=None), dict(Y=None), dict(gamma=None), dict(beta=None), dict(M=0), dict(F=0), dict(ldx=F - 1),
                dict(act=2), dict(act=-1), dict(train=0, rm=None, rv=None), dict(train=1, M=1), dict(rm=None),
                dict(rv=None), dict(sm=None), dict(si=None)):
        assert fwd(**bad) == E_ARG, bad
    assert fwd(train=0, M=1) == 0          # eval mode takes a single row

    sm, si, dY = t(F), t(F) + 1, t(M, F)

    def bwd(**o):
        w = _ws()
        a = dict(dY=dY, Y=X, X=X, sm=sm, si=si, gamma=gamma, dX=t(M, F), dg=t(F), db=t(F), ws=w, wsb=w.numel(), M=M,
                 F=F, act=1)
        a.update(o)
        return _bn_bwd_call(a, rc_only=True)

    assert bwd() == 0
    ws = _ws()
    for bad in (dict(dY=None), dict(X=None), dict(sm=None), dict(si=None), dict(gamma=None), dict(dX=None), dict(M=0),
                dict(F=0), dict(act=2), dict(act=-1), dict(act=1, Y=None),
                dict(dg=None, wsp=None), dict(db=None, wsp=None), dict(dg=None, db=None, wsp=None),
                dict(dg=None, wsb=2 * 4 * F - 1), dict(dg=None, wsp=ws.data_ptr() + 4, wsb=1024)):
        assert bwd(**bad) == E_ARG, bad
    assert bwd(act=0, Y=None) == 0
    assert bwd(dg=None) == 0 and bwd(db=None) == 0     # one of the pair missing: the workspace takes it
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------
# activations
ACT_N = [0, 1, 255, 257, 4096 * 256 + 3]     # the last wraps the grid-stride loop (4096 blocks of 256)
SPECIAL = [0.0, -0.0, 1e-30, -1e-30, 88.0, -88.0, 104.0, -104.0, float("inf"), float("-inf")]


def _act_x(n, seed=0):
    """uniform on [-30, 30], the explicit edge values at the end (as far as n allows)"""
    g = torch.Generator().manual_seed(seed + n)
    x = (torch.rand(n, generator=g) * 60 - 30).float()
    k = min(n, len(SPECIAL))
    if k:
        x[n - k:] = torch.tensor(SPECIAL[:k])
    return x


def _act_fwd(x, act, inplace=False):
    C = _C()
    n = x.numel()
    X = torch.full((n + 8,), -7.0, device="cuda")
    X[:n] = x.cuda()
    Y = X if inplace else torch.full((n + 8,), -7.0, device="cuda")
    C.check(C.lib.cgl_act_fwd(_p(X), n, act, SLOPE, _p(Y), _s()), "cgl_act_fwd")
    torch.cuda.synchronize()
    assert (Y[n:] == -7.0).all(), "stores past n"
    return Y[:n].cpu()


def _act_bwd(g, y, act, inplace=False):
    C = _C()
    n = g.numel()
    G = torch.full((n + 8,), -7.0, device="cuda")
    G[:n] = g.cuda()
    Yd = torch.empty(max(n, 1), device="cuda")
    Yd[:n] = y.cuda()
    D = G if inplace else torch.full((n + 8,), -7.0, device="cuda")
    C.check(C.lib.cgl_act_bwd(_p(G), _p(Yd), n, act, SLOPE, _p(D), _s()), "cgl_act_bwd")
    torch.cuda.synchronize()
    assert (D[n:] == -7.0).all(), "stores past n"
    return D[:n].cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _leaky32(x, sel=None):
    sel = x if sel is None else sel
    return torch.where(sel > 0, x, x * torch.tensor(SLOPE, dtype=torch.float32))    # one fp32 multiply


@pytest.mark.parametrize("n", ACT_N)
@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_act_fwd(act, n):
    """act 0: bitwise copy.  LeakyReLU: bitwise x or fp32(x slope).  Tanh: the kernel evaluates in double and
    rounds once; asserted EQUAL to the correctly rounded fp32 of fp64 tanh (seen on the MI355X: equal at all
    1 048 579 values, so the <= 1 ulp fallback is not used).  Sigmoid on [-30, 30]: expf within 2 ulp, one add, one
    divide -> |y - ref| <= 8 u ref (measured 0.31 of it); exactly 0 / 1 at -inf / +inf, inside [0, 1] elsewhere."""
    x = _act_x(n)
    y = _act_fwd(x, act)
    assert torch.equal(_bits(_act_fwd(x, act, inplace=True)), _bits(y)), "in-place (Y == X) differs"
    if n == 0:
        return
    if act == 0:
        assert torch.equal(_bits(y), _bits(x))
    elif act == 1:
        assert torch.equal(_bits(y), _bits(_leaky32(x)))
    elif act == 2:
        ref = torch.tanh(x.double()).float()
        nd = int((_bits(y) != _bits(ref)).sum())
        print(f"act_fwd tanh n={n}: {nd} values differ from the correctly rounded fp32 tanh")
        assert torch.equal(_bits(y), _bits(ref))
    else:
        assert not torch.isnan(y).any() and (y >= 0).all() and (y <= 1).all()
        assert (y[x == float("inf")] == 1).all() and (y[x == float("-inf")] == 0).all()
        inr = x.abs() <= 30
        ref = 1.0 / (1.0 + torch.exp(-x[inr].double()))
        rat = float(((y[inr].double() - ref).abs() / (8 * U * ref)).max())
        print(f"act_fwd sigmoid n={n}: worst ratio to bound {rat:.3f}")
        assert rat <= 1.0


@pytest.mark.parametrize("n", ACT_N)
@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_act_bwd(act, n):
    """Backward from the activation OUTPUT y.  LeakyReLU: bitwise g or fp32(g slope).  Tanh: within 1 ulp of
    fp64 g (1 - y^2) (evaluated in double, rounded once).  Sigmoid: |d - ref| <= 4 u |g| y (1 - y) + u |g| y (the
    second term: the rounding of 1 - y, which does not shrink with 1 - y near y = 1).  Measured on the MI355X:
    Tanh 0.50 ulp, Sigmoid 0.49 of its bound."""
    x = _act_x(n, seed=9)
    gg = torch.randn(n, generator=torch.Generator().manual_seed(n + 31))
    if act == 2:
        y = torch.tanh(x.double()).float()
    elif act == 3:
        y = (1.0 / (1.0 + torch.exp(-x.double()))).float()
    else:
        y = x
    d = _act_bwd(gg, y, act)
    assert torch.equal(_bits(_act_bwd(gg, y, act, inplace=True)), _bits(d)), "in-place (dX == dY) differs"
    if n == 0:
        return
    g64, y64 = gg.double(), y.double()
    if act == 0:
        assert torch.equal(_bits(d), _bits(gg))
    elif act == 1:
        assert torch.equal(_bits(d), _bits(_leaky32(gg, sel=y)))
    elif act == 2:
        ref = g64 * (1.0 - y64 * y64)
        rat = float(((d.double() - ref).abs() / _ulp32(ref)).max())
        print(f"act_bwd tanh n={n}: worst error {rat:.3f} ulp")
        assert rat <= 1.0
    else:
        ref = g64 * (y64 * (1.0 - y64))
        # (+ one fp32 denormal step: below the normal range a rounding is absolute, not relative)
        bound = 4 * U * g64.abs() * y64 * (1.0 - y64) + U * g64.abs() * y64 + 2.0 ** -149
        err = (d.double() - ref).abs()
        assert torch.isfinite(d).all()
        assert (err[bound == 0] == 0).all()
        nz = bound > 0
        rat = float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
        print(f"act_bwd sigmoid n={n}: worst ratio to bound {rat:.3f}")
        assert rat <= 1.0


def test_act_bad_arguments():
    C = _C()
    x = torch.zeros(8, device="cuda")
    for act in (-1, 4):
        assert C.lib.cgl_act_fwd(_p(x), 8, act, SLOPE, _p(x), _s()) == E_ARG
        assert C.lib.cgl_act_bwd(_p(x), _p(x), 8, act, SLOPE, _p(x), _s()) == E_ARG
    assert C.lib.cgl_act_fwd(None, 8, 1, SLOPE, _p(x), _s()) == E_ARG
    assert C.lib.cgl_act_fwd(_p(x), 8, 1, SLOPE, None, _s()) == E_ARG
    assert C.lib.cgl_act_fwd(_p(x), -1, 1, SLOPE, _p(x), _s()) == E_ARG
    assert C.lib.cgl_act_bwd(None, _p(x), 8, 1, SLOPE, _p(x), _s()) == E_ARG
    assert C.lib.cgl_act_bwd(_p(x), None, 8, 1, SLOPE, _p(x), _s()) == E_ARG
    assert C.lib.cgl_act_bwd(_p(x), _p(x), 8, 1, SLOPE, None, _s()) == E_ARG
    assert C.lib.cgl_act_bwd(_p(x), _p(x), -1, 1, SLOPE, _p(x), _s()) == E_ARG
