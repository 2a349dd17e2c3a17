"""The fp32 dispatch routes of the 3x3 convolution kernels (csrc/cgl_conv.hip) against a plain fp64 reference.

launch_conv_mma / conv_fwd_impl / conv_bwd_data_impl / conv_bwd_weight_impl pick one of about forty kernel and
template variants per call.  Each case below names the route it is written for, and the test asserts that route from
the library's own launch record (conv_ops.last_launches: what the launch sites stored, not a model of the
selection); a coverage test per direction holds the tables to a literal list of routes, so a removed case fails.

Two kinds of input per case:

* exact -- x, w, b, dy are integers in -2..2, dropout scales 0 or 2, slopes 0.25 / 0.5, folded-BatchNorm scales in
  {0.5, 1, 2} with integer shifts.  Every product and partial sum is then a multiple of 2^-4 below 2^20 in magnitude
  (the longest sum here, 457,728 pixels of |x dy| <= 4, stays below 2^21 in whole numbers), so it has at most 24
  significant bits and fp32 arithmetic is exact in any order (the phase-combined weights of the upsampling conv are
  sums of at most four such integers; every operand fits bf16's 8 significant bits), and the result must EQUAL the
  fp64 reference.  A
  dropped, duplicated or misplaced term cannot pass at any M, where a worst-case rounding bound (which grows with
  the reduction length) would hide it.  Every MFMA case runs again under mma_dtype("bf16") against the same values,
  and the record must then carry the BF16 flag.
* rounded -- standard-normal data scaled as in test_gpu_conv_ops.py, each element bounded by
  |got - ref| <= (K + 8) 2^-24 A, A the same operation on absolute values in fp64 (conv2d(|x|, |w|) + |b|, times
  |drop|) and K the products accumulated into the element: forward 9 cin (the phase form of the upsampling conv
  accumulates 4 cin products of weights that are sums of up to four: 4 cin + 3 roundings, below 9 cin + 8), input
  gradient 9 cout (16 cout for the upsampling conv), weight gradient n ho wo.  Tanh: the bound passes through its
  Lipschitz constant 1, plus 4 2^-24 |y|.  The worst ratio to the bound is printed per case.

Outputs are NaN-filled and followed by canary words (test_gpu_conv_stats_canary.py's padded / canary_ok).
"""
import os

import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_stats_canary import canary_ok, padded

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
MFMA = ("cgl_conv_fwd", "cgl_conv_fwd_halo", "cgl_conv_wgrad", "cgl_conv_wgrad_lds")


def ops():
    from cglgan import conv_ops
    return conv_ops


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def route(l):
    """The route a launch record names: kernel, template arguments and (MFMA forward) the workgroup's waves."""
    t = "".join("," + f for f in ("FAST", "ROW", "STAGE", "BNIN", "LDSM") if f in l.flags)
    if l.kernel == "cgl_conv_fwd":
        return f"cgl_conv_fwd<{l.tm},{l.tn}{t}> {l.wm}x{l.wn}x{l.wk}"
    if l.kernel == "cgl_conv_wgrad":
        return f"cgl_conv_wgrad<{l.tm},{l.tn}{t}>"
    if l.kernel == "cgl_conv_wgrad_lds":
        return f"cgl_conv_wgrad_lds<{l.wm},{l.wn},{l.wk}{t}>"
    if l.kernel in ("cgl_conv_n1_tile", "cgl_conv_wgrad_n1t"):
        return f"{l.kernel}<{l.tm},{l.tn}{t}>"
    return l.kernel + t


def main_launch(ls):
    ls = [l for l in ls if l.kernel != "cgl_conv_pack"]
    assert ls, "nothing but the pack was launched"
    return ls[0]


def draw(shape, g, exact, scale=1.0):
    if exact:
        return torch.randint(-2, 3, shape, generator=g).double()
    return torch.randn(shape, generator=g, dtype=torch.float64) * scale


def draw_drop(n, c, g, exact):
    keep = torch.rand(n, c, generator=g) < 0.75
    return keep.double() * (2.0 if exact else 1 / 0.75)


def bn_coef(groups, cin, g, exact):
    """[2][groups][cin] fp32 scale / shift of a folded BatchNorm (bn2d_fwd_stats(coef=)'s layout)"""
    if exact:
        sc = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (groups, cin), generator=g)]
        sh = torch.randint(-1, 2, (groups, cin), generator=g).float()
    else:
        sc = 0.5 + torch.rand(groups, cin, generator=g)
        sh = 0.3 * torch.randn(groups, cin, generator=g)
    return torch.stack([sc, sh]).float().contiguous()


def bn_apply64(x, coef, groups, slope, group=None):
    """LeakyReLU(fmaf(x, scale, shift)) in fp64 from the fp32 coefficients; x NCHW fp64, images stacked by group
    (group given: every image is of that forward call)"""
    n, cin = x.shape[0], x.shape[1]
    c = coef.double()
    gi = torch.full((n,), group) if group is not None else torch.arange(n) // (n // groups)
    v = x * c[0][gi][:, :, None, None] + c[1][gi][:, :, None, None]
    return torch.where(v > 0, v, v * slope)


def conv64(x, w, b, stride, up):
    if up:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    return F.conv2d(x, w, b, stride, 1)


def check(got, ref, bound, exact, what, worst):
    """exact: got == ref; else |got - ref| <= bound elementwise (records the worst ratio)"""
    got = got.detach().double().cpu()
    assert not torch.isnan(got).any(), f"{what}: NaN left in the output"
    if exact:
        bad = int((got != ref).sum())
        assert bad == 0, f"{what}: {bad} of {ref.numel()} elements differ from the exact reference " \
                         f"(max |diff| {float((got - ref).abs().max()):.3g})"
        return
    ratio = float(((got - ref).abs() / bound.clamp_min(1e-300)).max())
    worst[what] = max(worst.get(what, 0.0), ratio)
    assert ratio <= 1.0, f"{what}: error {ratio:.3f} x the bound"


class EnvSet:
    def __init__(self, env):
        self.env, self.old = env or {}, {}

    def __enter__(self):
        for k, v in self.env.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---------------------------------------------------------------------------------------------------------------
# Forward.  (route, (n, h, w, cin, cout, stride, up), act, options): options "bnin" = in_groups of the folded
# BatchNorm, "env" = the documented switches that select the route, "drop" = a Dropout2d scale in the epilogue.
# Ragged last tiles in M and in N: the 32 x 32 cases (M = 60 / 30 / 15 x 4 of 32, N = 20 / 24 of 32), 64 x 64
# (M = 16337 of 64, N = 96 of 64), 64 x 32 and 256 x 32 (N = 24 of 32: these tilings are chosen for N <= 32, so their
# one tile in N is the ragged one), 128 x 128 (N = 192 of 128, M = 32736 of 128), 256 x 64 (N = 48 of 64,
# M = 131967 / 134310 of 256).
FWD = [
    ("cgl_conv_fwd<1,1> 1x1x4", (2, 6, 5, 12, 20, 1, 0), 1, dict(drop=True)),
    ("cgl_conv_fwd<1,1> 1x1x4", (2, 7, 5, 3, 24, 2, 0), 0, {}),
    ("cgl_conv_fwd<1,1> 1x1x4", (1, 5, 3, 12, 20, 1, 1), 1, {}),
    ("cgl_conv_fwd<1,1> 1x1x4", (3, 7, 9, 3, 1, 1, 0), 2, {}),                    # N = 1 on the MFMA kernel
    ("cgl_conv_fwd<1,1> 1x1x4", (2, 9, 7, 1, 12, 1, 0), 1, {}),                   # Cin = 1 that c1_ok refuses (cout 12)
    # ... and Tanh, which alone keeps cout 16 off the vector kernel: no exact form (those drop the Tanh)
    ("cgl_conv_fwd<1,1> 1x1x4", (2, 9, 7, 1, 16, 1, 0), 2, dict(rounded_only=True)),
    ("cgl_conv_fwd<1,1,FAST> 1x1x4", (2, 9, 7, 32, 48, 1, 0), 1, dict(drop=True)),
    ("cgl_conv_fwd<1,1,FAST> 1x1x4", (9, 16, 16, 16, 96, 1, 1), 0, {}),           # tiled upsampling conv, no halo
    ("cgl_conv_fwd<2,2,FAST> 1x1x4", (17, 31, 31, 16, 96, 1, 0), 1, {}),          # 64 x 64
    ("cgl_conv_fwd<2,2> 1x1x4", (17, 31, 31, 12, 96, 1, 0), 0, {}),
    ("cgl_conv_fwd<2,1,FAST> 1x1x4", (33, 31, 32, 16, 24, 1, 0), 1, {}),          # 64 x 32
    ("cgl_conv_fwd<2,1> 1x1x4", (33, 31, 32, 12, 24, 1, 0), 0, {}),
    ("cgl_conv_fwd<2,2,FAST,LDSM> 2x2x1", (33, 31, 32, 16, 192, 1, 0), 1, {}),    # 128 x 128
    ("cgl_conv_fwd<2,2,FAST> 2x2x1", (33, 31, 32, 16, 192, 1, 0), 0, dict(env={"CGL_CONV_LDSM": "0"})),
    ("cgl_conv_fwd<2,2> 2x2x1", (33, 31, 32, 12, 192, 1, 0), 0, {}),
    ("cgl_conv_fwd<2,2,FAST> 4x1x1", (129, 31, 33, 16, 48, 1, 0), 1, {}),         # 256 x 64
    ("cgl_conv_fwd<2,1,FAST> 4x1x1", (129, 31, 33, 16, 24, 1, 0), 0, {}),         # 256 x 32
    ("cgl_conv_fwd_halo", (1, 8, 8, 16, 64, 1, 1), 1, {}),
    ("cgl_conv_fwd_halo", (2, 8, 8, 16, 128, 1, 1), 0, {}),
    ("cgl_conv_n1", (2, 6, 10, 16, 1, 2, 0), 2, {}),
    ("cgl_conv_n1", (2, 6, 10, 16, 1, 1, 1), 0, {}),
    ("cgl_conv_n1_tile<0,0>", (2, 21, 32, 16, 1, 1, 0), 2, {}),                   # OH = 21 ragged against CGL_N1T_TH
    ("cgl_conv_n1_tile<0,0>", (3, 7, 9, 64, 1, 1, 0), 0, {}),
    ("cgl_conv_n1_tile<16,32>", (2, 20, 32, 64, 1, 1, 0), 2, dict(env={"CGL_N1_TILE": "1"})),
    ("cgl_conv_n1_part", (2, 20, 32, 64, 1, 1, 0), 2, {}),
    ("cgl_conv_c1_fwd", (2, 9, 7, 1, 4, 1, 0), 1, dict(drop=True)),
    ("cgl_conv_c1_fwd", (2, 9, 7, 1, 4, 2, 0), 0, {}),
    ("cgl_conv_c1_fwd", (3, 11, 9, 1, 8, 1, 0), 0, {}),                           # npix 297: not a multiple of 256
    ("cgl_conv_c1_fwd", (2, 9, 7, 1, 8, 2, 0), 1, {}),
    ("cgl_conv_c1_fwd", (2, 9, 7, 1, 16, 1, 0), 1, {}),
    ("cgl_conv_c1_fwd", (3, 32, 32, 1, 16, 2, 0), 1, dict(drop=True)),
    # the input's BatchNorm + LeakyReLU folded into the operand load
    ("cgl_conv_fwd<1,1,FAST,BNIN> 1x1x4", (2, 6, 5, 16, 20, 1, 0), 1, dict(bnin=2)),
    ("cgl_conv_fwd<2,1,FAST,BNIN> 1x1x4", (33, 31, 32, 16, 24, 1, 0), 0, dict(bnin=1)),
    ("cgl_conv_fwd<2,2,FAST,BNIN> 1x1x4", (17, 31, 31, 16, 96, 1, 0), 1, dict(bnin=1)),
    ("cgl_conv_fwd<2,2,FAST,BNIN> 2x2x1", (34, 31, 32, 16, 192, 1, 0), 0, dict(bnin=2)),
    ("cgl_conv_fwd<2,2,FAST,BNIN> 4x1x1", (130, 31, 33, 16, 48, 1, 0), 1, dict(bnin=2)),
    ("cgl_conv_fwd<2,1,FAST,BNIN> 4x1x1", (130, 31, 33, 16, 24, 1, 0), 0, dict(bnin=2)),
    ("cgl_conv_fwd_halo,BNIN", (2, 8, 8, 16, 128, 1, 1), 0, dict(bnin=2)),
    ("cgl_conv_n1_part,BNIN", (2, 20, 32, 64, 1, 1, 0), 2, dict(bnin=2)),
]

# one entry per fp32 instantiation launch_conv_mma / conv_fwd_impl can launch for a forward, the MFMA ones per
# workgroup tiling (32 x 32, 64 x 64, 64 x 32, 128 x 128 with and without LDSM, 256 x 64, 256 x 32)
FWD_ROUTES = [
    "cgl_conv_fwd<1,1> 1x1x4", "cgl_conv_fwd<1,1,FAST> 1x1x4", "cgl_conv_fwd<2,1> 1x1x4",
    "cgl_conv_fwd<2,1,FAST> 1x1x4", "cgl_conv_fwd<2,2> 1x1x4", "cgl_conv_fwd<2,2,FAST> 1x1x4",
    "cgl_conv_fwd<2,2> 2x2x1", "cgl_conv_fwd<2,2,FAST> 2x2x1", "cgl_conv_fwd<2,2,FAST,LDSM> 2x2x1",
    "cgl_conv_fwd<2,2,FAST> 4x1x1", "cgl_conv_fwd<2,1,FAST> 4x1x1",
    "cgl_conv_fwd<1,1,FAST,BNIN> 1x1x4", "cgl_conv_fwd<2,1,FAST,BNIN> 1x1x4", "cgl_conv_fwd<2,2,FAST,BNIN> 1x1x4",
    "cgl_conv_fwd<2,2,FAST,BNIN> 2x2x1", "cgl_conv_fwd<2,2,FAST,BNIN> 4x1x1", "cgl_conv_fwd<2,1,FAST,BNIN> 4x1x1",
    "cgl_conv_fwd_halo", "cgl_conv_fwd_halo,BNIN", "cgl_conv_n1", "cgl_conv_n1_part", "cgl_conv_n1_part,BNIN",
    "cgl_conv_n1_tile<0,0>", "cgl_conv_n1_tile<16,32>", "cgl_conv_c1_fwd",
]


def _fwd_inputs(case, exact):
    rt, (n, h, w, cin, cout, stride, up), act, opt = case
    g = torch.Generator().manual_seed(hash((n, h, w, cin, cout, stride, up, exact)) % (1 << 31))
    x = draw((n, cin, h, w), g, exact)
    wt = draw((cout, cin, 3, 3), g, exact, 1 / (3 * cin ** 0.5))
    b = draw((cout,), g, exact, 0.1)
    drop = draw_drop(n, cout, g, exact) if opt.get("drop") else None
    coef = bn_coef(opt["bnin"], cin, g, exact) if opt.get("bnin") else None
    return x, wt, b, drop, coef


def _fwd_ref(case, exact, x, wt, b, drop, coef, slope, in_slope):
    rt, (n, h, w, cin, cout, stride, up), act, opt = case
    xin = bn_apply64(x, coef, opt["bnin"], in_slope) if coef is not None else x
    pre = conv64(xin, wt, b, stride, up)
    bound = 0.0 if exact else (9 * cin + 8) * U * conv64(xin.abs(), wt.abs(), b.abs(), stride, up)
    if act == 1:
        ref = torch.where(pre > 0, pre, pre * slope)
    elif act == 2:
        ref = torch.tanh(pre)
        bound = bound + 4 * U * ref.abs()
    else:
        ref = pre
    if drop is not None:
        ref = ref * drop[:, :, None, None]
        bound = bound * drop[:, :, None, None]
    return ref, bound


WORST = {}


def _params(table):
    return [pytest.param(i, e, id=f"{i}-{c[0]}-{'exact' if e else 'rounded'}") for i, c in enumerate(table)
            for e in (True, False) if not (e and c[-1].get("rounded_only"))]


@pytest.mark.parametrize("ci,exact", _params(FWD))
def test_fwd_route(ci, exact):
    O = ops()
    case = FWD[ci]
    rt, (n, h, w, cin, cout, stride, up), act, opt = case
    if exact and act == 2:
        act, case = 0, (rt, case[1], 0, opt)          # exact cases: activation none or LeakyReLU
    slope, in_slope = (0.25, 0.5) if exact else (0.2, 0.2)
    x, wt, b, drop, coef = _fwd_inputs(case, exact)
    ref, bound = _fwd_ref(case, exact, x, wt, b, drop, coef, slope, in_slope)
    ho, wo = O.conv_out_hw(h, w, stride, up)
    xd, wd, bd = nhwc(x).float().to(DEV), wt.float().to(DEV), b.float().to(DEV)
    dd = drop.float().to(DEV).contiguous() if drop is not None else None
    kw = {}
    if coef is not None:
        pk = O.PackSet()
        pk.add("x", "f", wd, h, w, cin, cout, stride, up)
        pk.finalize(xd.device).run()
        kw = dict(wp=pk["f"], bn_in=(coef.to(DEV), opt["bnin"], O.ACT_LEAKY, in_slope))
    worst = {}
    for dt in (["f32", "bf16"] if exact else ["f32"]):
        y, ybuf = padded(n * ho * wo * cout)
        y.fill_(float("nan"))
        with EnvSet(opt.get("env")), O.mma_dtype(dt):
            O.conv3x3_fwd(xd, wd, bd, y, n, h, w, cin, cout, stride, up, act, slope, dd, **kw)
            ml = main_launch(O.last_launches())
        torch.cuda.synchronize()
        assert route(ml) == rt, f"case written for {rt} ran {route(ml)}"
        if dt == "bf16":
            if ml.kernel not in MFMA:
                break                                  # the vector kernels ignore the mode: nothing to repeat
            assert "BF16" in ml.flags
        else:
            assert "BF16" not in ml.flags
        canary_ok(ybuf, y.numel(), f"{rt} y ({dt})")
        check(nchw(y.view(n, ho, wo, cout)), ref, bound, exact, f"fwd {rt} {case[1]} ({dt})", worst)
    for k, v in worst.items():
        WORST[k] = v
        print(f"{k}: worst error / bound = {v:.3f}")


def test_fwd_routes_covered():
    assert sorted({c[0] for c in FWD}) == sorted(FWD_ROUTES)


# ---------------------------------------------------------------------------------------------------------------
# Input gradient: dX of the convolution (n, h, w, cin -> cout) from dY; its GEMM has N = cin and K = taps cout.
BWD = [
    ("cgl_conv_fwd<1,1> 1x1x4", (2, 6, 5, 20, 12, 1, 0), {}),                     # cout % 16 != 0: non-FAST
    ("cgl_conv_fwd<1,1> 1x1x4", (2, 7, 5, 24, 3, 2, 0), {}),                      # stride 2: 4 parity problems
    ("cgl_conv_fwd<1,1> 1x1x4", (1, 5, 3, 20, 12, 1, 1), {}),                     # upsampling conv: 16 taps
    ("cgl_conv_fwd<1,1> 1x1x4", (2, 6, 5, 32, 1, 1, 0), {}),                      # cout = 1: K = 9, Kp = 16
    ("cgl_conv_fwd<1,1,FAST> 1x1x4", (2, 7, 7, 32, 64, 2, 0), {}),
    ("cgl_conv_fwd<1,1,FAST> 1x1x4", (9, 16, 16, 96, 16, 1, 1), {}),              # tiled upsampling conv
    ("cgl_conv_fwd<2,1> 1x1x4", (40, 32, 32, 16, 24, 2, 0), dict(ilv=True)),      # stride 2 tiled, even dims: ILV
    ("cgl_conv_fwd<2,1> 1x1x4", (40, 31, 33, 16, 24, 2, 0), dict(ilv=False)),     # odd dims: no ILV
    ("cgl_conv_fwd<2,1,FAST> 1x1x4", (33, 31, 32, 24, 16, 1, 0), {}),
    ("cgl_conv_fwd<2,2,FAST> 1x1x4", (17, 31, 31, 96, 16, 1, 0), {}),             # N = cin = 96: ragged of 64
    ("cgl_conv_fwd<2,2,FAST,LDSM> 2x2x1", (33, 31, 32, 192, 16, 1, 0), {}),
    ("cgl_conv_fwd<2,2> 2x2x1", (33, 31, 32, 192, 12, 1, 0), {}),
    ("cgl_conv_fwd<2,2,FAST> 4x1x1", (129, 31, 33, 48, 16, 1, 0), {}),
    ("cgl_conv_fwd<2,1,FAST> 4x1x1", (129, 31, 33, 24, 16, 1, 0), {}),
    ("cgl_conv_n1", (2, 9, 7, 1, 16, 2, 0), {}),                                  # D Conv2d(1, 16, s2)'s input gradient
    ("cgl_conv_n1", (2, 9, 7, 1, 16, 1, 0), {}),
    ("cgl_conv_bwd_n1", (3, 7, 9, 64, 1, 1, 0), {}),
]

BWD_ROUTES = [
    "cgl_conv_fwd<1,1> 1x1x4", "cgl_conv_fwd<1,1,FAST> 1x1x4", "cgl_conv_fwd<2,1> 1x1x4",
    "cgl_conv_fwd<2,1,FAST> 1x1x4", "cgl_conv_fwd<2,2,FAST> 1x1x4", "cgl_conv_fwd<2,2> 2x2x1",
    "cgl_conv_fwd<2,2,FAST,LDSM> 2x2x1", "cgl_conv_fwd<2,2,FAST> 4x1x1", "cgl_conv_fwd<2,1,FAST> 4x1x1",
    "cgl_conv_n1", "cgl_conv_bwd_n1",
]


def _grads64(x, wt, dy, stride, up, wrt):
    xr, wr = x.clone().requires_grad_(wrt == "x"), wt.clone().requires_grad_(wrt == "w")
    conv64(xr, wr, None, stride, up).backward(dy)
    return xr.grad if wrt == "x" else wr.grad


@pytest.mark.parametrize("ci,exact", _params(BWD))
def test_bwd_data_route(ci, exact):
    O = ops()
    rt, (n, h, w, cin, cout, stride, up), opt = BWD[ci]
    g = torch.Generator().manual_seed(hash((n, h, w, cin, cout, stride, up, exact, 1)) % (1 << 31))
    ho, wo = O.conv_out_hw(h, w, stride, up)
    wt = draw((cout, cin, 3, 3), g, exact, 1 / (3 * cout ** 0.5))
    dy = draw((n, cout, ho, wo), g, exact)
    x0 = torch.zeros(n, cin, h, w, dtype=torch.float64)
    ref = _grads64(x0, wt, dy, stride, up, "x")
    bound = None if exact else ((16 if up else 9) * cout + 8) * U * _grads64(x0, wt.abs(), dy.abs(), stride, up, "x")
    wd, dyd = wt.float().to(DEV), nhwc(dy).float().to(DEV)
    worst = {}
    for dt in (["f32", "bf16"] if exact else ["f32"]):
        dx, dxbuf = padded(n * h * w * cin)
        dx.fill_(float("nan"))
        with O.mma_dtype(dt):
            O.conv3x3_bwd_data(dyd, wd, dx, n, h, w, cin, cout, stride, up)
            ml = main_launch(O.last_launches())
        torch.cuda.synchronize()
        assert route(ml) == rt, f"case written for {rt} ran {route(ml)}"
        if "ilv" in opt:
            assert ("ILV" in ml.flags) == opt["ilv"] and ml.np == 4
        if dt == "bf16":
            if ml.kernel not in MFMA:
                break
            assert "BF16" in ml.flags
        canary_ok(dxbuf, dx.numel(), f"{rt} dx ({dt})")
        check(nchw(dx.view(n, h, w, cin)), ref, bound, exact, f"bwd_data {rt} {BWD[ci][1]} ({dt})", worst)
    for k, v in worst.items():
        WORST[k] = v
        print(f"{k}: worst error / bound = {v:.3f}")


def test_bwd_data_routes_covered():
    assert sorted({c[0] for c in BWD}) == sorted(BWD_ROUTES)


# ---------------------------------------------------------------------------------------------------------------
# Weight and bias gradient.  (route, geometry, bias route, options).  Bias routes: "col" = the im2col ones-column of
# the MFMA kernel (BIAS_COL on its record and on the reduction's), "chan4" / "chan" = column sums by
# cgl_chan_reduce4 / cgl_chan_reduce (mode 2) + cgl_bn_finalize, "colsum_k" = cgl_colsum_k + cgl_bn_finalize,
# "c1" = inside the one-input-channel kernel.  Every case also runs with db = None.
WGRAD = [
    ("cgl_conv_wgrad<1,1,ROW>", (2, 8, 8, 2, 16, 1, 0), "col", dict(splits=2)),
    ("cgl_conv_wgrad<1,1>", (2, 7, 5, 3, 16, 1, 0), "col", dict(splits=1)),
    ("cgl_conv_wgrad<2,1,ROW>", (2, 8, 8, 2, 48, 1, 0), "col", {}),
    ("cgl_conv_wgrad<2,1>", (2, 7, 5, 3, 48, 1, 0), "col", {}),
    ("cgl_conv_wgrad<1,2,ROW>", (2, 8, 8, 12, 16, 1, 0), "col", {}),
    ("cgl_conv_wgrad<1,2>", (2, 7, 5, 12, 16, 2, 0), "col", {}),
    ("cgl_conv_wgrad<2,2,ROW>", (2, 8, 8, 12, 48, 1, 1), "col", {}),              # upsampling conv: 4 problems
    ("cgl_conv_wgrad<2,2>", (2, 7, 5, 12, 48, 1, 0), "col", {}),
    ("cgl_conv_wgrad<2,2,ROW>", (5, 32, 32, 64, 96, 1, 0), "colsum_k", {}),       # K % 64 == 0, 2^28 MACs, cout 96
    ("cgl_conv_wgrad<2,2,ROW>", (8, 32, 32, 64, 64, 1, 0), "chan4", {}),
    # the input's BatchNorm + LeakyReLU folded into the operand loads: bnin = (groups, group), group -1 = stacked
    # calls.  The folded form needs cin % 4 == 0, so TN = 1 (K + bias column <= 32) is the upsampling conv at cin 4
    ("cgl_conv_wgrad<1,1,ROW,BNIN>", (2, 8, 8, 4, 16, 1, 1), "col", dict(bnin=(1, 0))),
    ("cgl_conv_wgrad<1,1,BNIN>", (2, 7, 5, 4, 16, 1, 1), "col", dict(bnin=(2, 1))),
    ("cgl_conv_wgrad<2,1,ROW,BNIN>", (2, 8, 8, 4, 48, 1, 1), "col", dict(bnin=(2, 0))),
    ("cgl_conv_wgrad<2,1,BNIN>", (2, 7, 5, 4, 48, 1, 1), "col", dict(bnin=(1, 0))),
    ("cgl_conv_wgrad<1,2,ROW,BNIN>", (2, 8, 8, 12, 16, 1, 0), "col", dict(bnin=(2, 1))),
    ("cgl_conv_wgrad<1,2,BNIN>", (2, 7, 5, 12, 16, 1, 0), "col", dict(bnin=(1, 0))),
    ("cgl_conv_wgrad<2,2,ROW,BNIN>", (2, 8, 8, 12, 48, 1, 0), "col", dict(bnin=(1, 0))),
    ("cgl_conv_wgrad<2,2,BNIN>", (4, 7, 5, 12, 48, 1, 0), "col", dict(bnin=(2, -1))),     # two stacked calls
    ("cgl_conv_wgrad_lds<2,2,1>", (16, 8, 8, 128, 128, 1, 1), "chan4", {}),
    ("cgl_conv_wgrad_lds<1,4,1>", (8, 16, 16, 128, 64, 1, 1), "chan4", {}),
    ("cgl_conv_wgrad_lds<2,2,1,BNIN>", (16, 8, 8, 128, 128, 1, 1), "chan4", dict(bnin=(1, 0))),
    ("cgl_conv_wgrad_lds<1,4,1,BNIN>", (8, 16, 16, 128, 64, 1, 1), "chan4", dict(bnin=(2, 1))),
    ("cgl_conv_wgrad_n1", (3, 7, 9, 12, 1, 1, 0), "chan", {}),
    ("cgl_conv_wgrad_n1", (2, 6, 5, 3, 1, 1, 0), "chan", {}),
    ("cgl_conv_wgrad_n1t<2,0>", (3, 8, 8, 16, 1, 1, 0), "chan", {}),
    ("cgl_conv_wgrad_n1t<1,32,STAGE>", (2, 32, 32, 64, 1, 1, 0), "chan", {}),
    ("cgl_conv_wgrad_n1t<1,32,STAGE,BNIN>", (2, 32, 32, 64, 1, 1, 0), "chan", dict(bnin=(2, 1))),
    ("cgl_conv_c1_wgrad", (2, 9, 7, 1, 4, 1, 0), "c1", {}),
    ("cgl_conv_c1_wgrad", (2, 9, 7, 1, 4, 2, 0), "c1", {}),
    ("cgl_conv_c1_wgrad", (3, 11, 9, 1, 8, 1, 0), "c1", {}),
    ("cgl_conv_c1_wgrad", (2, 9, 7, 1, 8, 2, 0), "c1", {}),
    ("cgl_conv_c1_wgrad", (2, 9, 7, 1, 16, 1, 0), "c1", {}),
    ("cgl_conv_c1_wgrad", (3, 32, 32, 1, 16, 2, 0), "c1", dict(actdrop=True)),
]

# The no-stage specialised cgl_conv_wgrad_n1t needs >= 447 images of 32 x 32 x 64 (test_wgrad_n1t_no_stage, exact
# inputs only), and the CGL_WGRAD_KS=2 forms of cgl_conv_wgrad_lds a process of their own (the switch is read once:
# test_wgrad_lds_ks2); both tables count towards the coverage list.
N1T_NO_STAGE = [("cgl_conv_wgrad_n1t<1,32>", False), ("cgl_conv_wgrad_n1t<1,32,BNIN>", True)]
WGRAD_KS2 = [
    ("cgl_conv_wgrad_lds<2,2,2>", (16, 8, 8, 128, 128, 1, 1), "chan4", {}),
    ("cgl_conv_wgrad_lds<1,4,2>", (8, 16, 16, 128, 64, 1, 1), "chan4", {}),
]

# one entry per fp32 instantiation conv_bwd_weight_impl can launch
WGRAD_ROUTES = [
    "cgl_conv_wgrad<1,1>", "cgl_conv_wgrad<1,1,ROW>", "cgl_conv_wgrad<2,1>", "cgl_conv_wgrad<2,1,ROW>",
    "cgl_conv_wgrad<1,2>", "cgl_conv_wgrad<1,2,ROW>", "cgl_conv_wgrad<2,2>", "cgl_conv_wgrad<2,2,ROW>",
    "cgl_conv_wgrad<1,1,BNIN>", "cgl_conv_wgrad<1,1,ROW,BNIN>", "cgl_conv_wgrad<2,1,BNIN>",
    "cgl_conv_wgrad<2,1,ROW,BNIN>", "cgl_conv_wgrad<1,2,BNIN>", "cgl_conv_wgrad<1,2,ROW,BNIN>",
    "cgl_conv_wgrad<2,2,BNIN>", "cgl_conv_wgrad<2,2,ROW,BNIN>",
    "cgl_conv_wgrad_lds<2,2,1>", "cgl_conv_wgrad_lds<1,4,1>", "cgl_conv_wgrad_lds<2,2,1,BNIN>",
    "cgl_conv_wgrad_lds<1,4,1,BNIN>", "cgl_conv_wgrad_lds<2,2,2>", "cgl_conv_wgrad_lds<1,4,2>",
    "cgl_conv_wgrad_n1", "cgl_conv_wgrad_n1t<2,0>", "cgl_conv_wgrad_n1t<1,32,STAGE>",
    "cgl_conv_wgrad_n1t<1,32,STAGE,BNIN>", "cgl_conv_wgrad_n1t<1,32>", "cgl_conv_wgrad_n1t<1,32,BNIN>",
    "cgl_conv_c1_wgrad",
]
BIAS_ROUTES = ["col", "chan4", "chan", "colsum_k", "c1"]


def _bias_route(ls):
    ks = [l.kernel for l in ls]
    if "cgl_conv_c1_wgrad" in ks:
        return "c1"
    red = [l for l in ls if l.kernel == "cgl_conv_wgrad_reduce"][0]
    if "BIAS_COL" in red.flags:
        assert "BIAS_COL" in ls[0].flags and "cgl_bn_finalize" not in ks
        return "col"
    assert ks[-1] == "cgl_bn_finalize" and ls[-1].tm == 2
    return {"cgl_chan_reduce4": "chan4", "cgl_chan_reduce": "chan", "cgl_colsum_k": "colsum_k"}[ks[-2]]


def _run_wgrad(case, exact):
    O = ops()
    rt, (n, h, w, cin, cout, stride, up), brt, opt = case
    g = torch.Generator().manual_seed(hash((n, h, w, cin, cout, stride, up, exact, 2)) % (1 << 31))
    ho, wo = O.conv_out_hw(h, w, stride, up)
    x = draw((n, cin, h, w), g, exact)
    dy = draw((n, cout, ho, wo), g, exact)
    slope = 0.5 if exact else 0.2
    kw, xin, dyin = {}, x, dy
    if opt.get("bnin"):
        groups, group = opt["bnin"]
        coef = bn_coef(groups, cin, g, exact)
        xin = bn_apply64(x, coef, groups, slope, None if group < 0 else group)
        kw = dict(bn_in=(coef.to(DEV), group, groups, O.ACT_LEAKY, slope))
    if opt.get("actdrop"):
        # dy is the gradient at the block's output: LeakyReLU + Dropout2d backward applied per loaded value
        post = draw((n, cout, ho, wo), g, exact)
        drop = draw_drop(n, cout, g, exact)
        dyin = dy * drop[:, :, None, None] * torch.where(post > 0, 1.0, slope)
        kw = dict(act_drop=(nhwc(post).float().to(DEV), drop.float().to(DEV).contiguous(), slope))
    w0 = torch.zeros(cout, cin, 3, 3, dtype=torch.float64)
    K = n * ho * wo
    ref_w = _grads64(xin, w0, dyin, stride, up, "w")
    bound_w = None if exact else (K + 8) * U * _grads64(xin.abs(), w0, dyin.abs(), stride, up, "w")
    ref_b, bound_b = dyin.sum((0, 2, 3)), (K + 8) * U * dyin.abs().sum((0, 2, 3))
    xd, dyd = nhwc(x).float().to(DEV), nhwc(dy).float().to(DEV)
    worst = {}
    for dt in (["f32", "bf16"] if exact else ["f32"]):
        for with_db in (True, False):
            dw, dwbuf = padded(cout * cin * 9)
            db, dbbuf = padded(cout)
            dw.fill_(float("nan"))
            db.fill_(float("nan"))
            with O.mma_dtype(dt):
                O.conv3x3_bwd_weight(dyd, xd, dw, db if with_db else None, n, h, w, cin, cout, stride, up, **kw)
                ls = O.last_launches()
            torch.cuda.synchronize()
            tag = f"wgrad {rt} {case[1]} ({dt}, db {with_db})"
            assert route(ls[0]) == rt, f"case written for {rt} ran {route(ls[0])}"
            if "splits" in opt and with_db:
                assert ls[0].splits == opt["splits"]
            if ls[0].kernel in MFMA:
                assert ("BF16" in ls[0].flags) == (dt == "bf16")
            if with_db:
                assert _bias_route(ls) == brt, f"{tag}: bias by {_bias_route(ls)}, case written for {brt}"
                check(db, ref_b, bound_b, exact, tag + " db", worst)
            else:
                assert [l.kernel for l in ls if l.kernel in ("cgl_chan_reduce", "cgl_chan_reduce4", "cgl_colsum_k",
                                                             "cgl_bn_finalize")] == []
                assert "BIAS_COL" not in ls[0].flags
                assert bool(torch.isnan(db).all()), f"{tag}: db = None, yet the buffer beside it was written"
            canary_ok(dwbuf, dw.numel(), tag + " dw")
            canary_ok(dbbuf, db.numel(), tag + " db")
            check(dw.view(cout, cin, 3, 3), ref_w, bound_w, exact, tag + " dw", worst)
        if ls[0].kernel not in MFMA:
            break
    for k, v in worst.items():
        WORST[k] = v
        print(f"{k}: worst error / bound = {v:.3f}")


@pytest.mark.parametrize("ci,exact", _params(WGRAD))
def test_wgrad_route(ci, exact):
    _run_wgrad(WGRAD[ci], exact)


def test_wgrad_routes_covered():
    assert sorted({c[0] for c in WGRAD + WGRAD_KS2} | {r for r, _ in N1T_NO_STAGE}) == sorted(WGRAD_ROUTES)
    assert sorted({c[2] for c in WGRAD}) == sorted(BIAS_ROUTES)
    assert {c[3].get("splits") for c in WGRAD} >= {1, 2}      # the split reduction with one and with several splits


@pytest.mark.parametrize("rt,bnin", N1T_NO_STAGE)
def test_wgrad_n1t_no_stage(rt, bnin):
    """The specialised cgl_conv_wgrad_n1t without the LDS stage: per_block + 2 OW + 2 > 512 input pixels per block.
    Past 256 images the plan has its 1024 splits, so a block takes n pixels and the stage stops at n + 66 > 512:
    n = 447 is the smallest (the launch record decides: STAGE is absent).  Exact inputs only: an fp64 reference of
    the 576 sums on the device is cheap where an fp64 autograd over 458 k pixels x 64 channels on the CPU is not.
    With the folded BatchNorm (scales 0.5 / 1, integer shifts, slope 0.5) the operand is a multiple of 0.25 of
    magnitude <= 3, so every partial sum is a multiple of 0.25 below 457,728 x 3 x 2 < 2^22: still exact in fp32."""
    O = ops()
    n, h, cin = 447, 32, 64
    g = torch.Generator(device=DEV).manual_seed(447)
    x = torch.randint(-2, 3, (n, h, h, cin), generator=g, device=DEV).double()
    dy = torch.randint(-2, 3, (n, h, h, 1), generator=g, device=DEV).double()
    kw, xin = {}, x
    if bnin:
        gc = torch.Generator().manual_seed(3)
        coef = torch.stack([torch.tensor([0.5, 1.0])[torch.randint(0, 2, (2, cin), generator=gc)],
                            torch.randint(-1, 2, (2, cin), generator=gc).float()]).contiguous().to(DEV)
        v = x * coef[0, 1].double() + coef[1, 1].double()          # forward call 1 of 2
        xin = torch.where(v > 0, v, v * 0.5)
        kw = dict(bn_in=(coef, 1, 2, O.ACT_LEAKY, 0.5))
    dw, dwbuf = padded(cin * 9)
    db, dbbuf = padded(1)
    dw.fill_(float("nan"))
    O.conv3x3_bwd_weight(dy.float(), x.float(), dw, db, n, h, h, cin, 1, 1, 0, **kw)
    ls = O.last_launches()
    assert route(ls[0]) == rt, route(ls[0])
    xp = F.pad(xin, (0, 0, 1, 1, 1, 1))
    ref = torch.empty(cin, 3, 3, dtype=torch.float64)
    for kh in range(3):
        for kx in range(3):
            ref[:, kh, kx] = (xp[:, kh:kh + h, kx:kx + h, :] * dy).sum((0, 1, 2)).cpu()
    torch.cuda.synchronize()
    canary_ok(dwbuf, dw.numel(), "n1t dw")
    canary_ok(dbbuf, db.numel(), "n1t db")
    assert torch.equal(dw.view(1, cin, 3, 3)[0].cpu().double(), ref)
    assert float(db[0]) == float(dy.sum())


def _ks2_child():
    """(child process of test_wgrad_lds_ks2, CGL_WGRAD_KS=2 in its environment)"""
    for case in WGRAD_KS2:
        _run_wgrad(case, True)
        _run_wgrad(case, False)
    print("KS2-OK")


def test_wgrad_lds_ks2():
    """cgl_conv_wgrad_lds<2,2,2> and <1,4,2> (CGL_WGRAD_KS=2: 512-thread workgroups of two halves over half as many
    splits).  The library reads the switch once per process, so the two cases -- exact, its bf16 repeat, and
    rounded, as every other weight-gradient case -- run in a child process started with it."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = %r\n"
            "import test_gpu_conv_routes as T\nT._ks2_child()\n") % [p for p in sys.path if p]
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, cwd=here,
                       env=dict(os.environ, CGL_WGRAD_KS="2"))
    print(r.stdout)
    assert r.returncode == 0 and "KS2-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------------
# Epilogue statistics at small sizes, on exact inputs, against an fp64 restatement of the partials.
def _chunk_stats(rows, counts):
    """{sum, M2 about the chunk mean} per 32-row chunk over its first counts[chunk] rows; rows [nrows, C] fp64"""
    out = torch.zeros(rows.shape[0] // 32, rows.shape[1], 2, dtype=torch.float64)
    for ch, cnt in enumerate(counts):
        blk = rows[ch * 32:ch * 32 + cnt]
        if cnt:
            out[ch, :, 0] = blk.sum(0)
            out[ch, :, 1] = ((blk - blk.mean(0)) ** 2).sum(0)
    return out


@pytest.mark.parametrize("nv", [None, 1, 3])
@pytest.mark.parametrize("groups", [1, 2])
def test_fwd_epilogue_stats_exact(groups, nv):
    """cgl_conv3x3_fwd_packed_stats, n = 4 images of 4 x 4 (16 rows each), 16 -> 32 channels (the smallest cout the
    epilogue takes), one and two stacked calls, with and without nvalid.  The epilogue sums the stored fp32 values
    and their squared deviations from the chunk mean in DOUBLE throughout (cgl_conv_fwd_body: sm, mu = sm / count, dd
    dd), and every chunk here counts 32, 16 or 0 real rows, so on exact inputs the mean and every term are exact:
    both words of every pair must EQUAL the fp64 restatement.  nvalid leaves a chunk half real (16 rows) or empty."""
    O = ops()
    n, h, cin, cout = 4, 4, 16, 32
    ng = n // groups
    if nv is not None and nv > ng:
        nv = ng                               # (a full first call given as nvalid: the plain chunks)
    g = torch.Generator().manual_seed(10 * groups + (nv or 0))
    x, wt, b = draw((n, cin, h, h), g, True), draw((cout, cin, 3, 3), g, True), draw((cout,), g, True)
    ref = conv64(x, wt, b, 1, 0)
    xd, wd, bd = nhwc(x).float().to(DEV), wt.float().to(DEV), b.float().to(DEV)
    pk = O.PackSet()
    pk.add("x", "f", wd, h, h, cin, cout)
    pk.finalize(xd.device).run()
    nch = O.stat_chunks(n, h, h, cin, cout, 1, 0, groups)
    assert nch == n * h * h // 32
    part, pbuf = padded(nch * cout * 2, torch.float64)
    y, ybuf = padded(n * h * h * cout)
    y.fill_(float("nan"))
    nvd = torch.tensor([nv], dtype=torch.int32, device=DEV) if nv is not None else None
    O.conv3x3_fwd(xd, None, bd, y, n, h, h, cin, cout, wp=pk["f"], stats=(part, groups), nvalid=nvd)
    ml = main_launch(O.last_launches())
    assert ml.kernel == "cgl_conv_fwd" and "STATS_FWD" in ml.flags and ("NVALID" in ml.flags) == (nv is not None)
    torch.cuda.synchronize()
    canary_ok(pbuf, part.numel(), "st_part")
    canary_ok(ybuf, y.numel(), "y")
    check(nchw(y.view(n, h, h, cout)), ref, None, True, "stats fwd y", {})
    rows = nhwc(ref).reshape(n * h * h, cout)
    real0 = (nv if nv is not None else ng) * h * h            # real rows of the first call
    counts = [min(max(real0 - ch * 32, 0), 32) if ch * 32 < ng * h * h else 32 for ch in range(nch)]
    want = _chunk_stats(rows, counts)
    got = part.view(nch, cout, 2).cpu()
    assert torch.equal(got[:, :, 0], want[:, :, 0]), "chunk sums"
    assert torch.equal(got[:, :, 1], want[:, :, 1]), "chunk M2"


@pytest.mark.parametrize("mode,groups", [("post", 1), ("post", 2), ("post_coef", 1), ("neither", 2)])
def test_bwd_epilogue_stats_exact(mode, groups):
    """cgl_conv3x3_bwd_data_packed_stats: {sum g, sum g (x - mean)} per 32-row chunk of dX, g = dX leaky'(post), with
    post, with post_coef and with neither.  The epilogue forms g and g (x - mean) in fp32 and sums them in double
    (S += (double)gg, D += (double)(gg * (xv - mu))): on exact inputs (integer x and mean, slope 0.25) both fp32
    steps are exact, so both words must EQUAL the fp64 restatement."""
    O = ops()
    n, h, cin, cout, slope = 4, 4, 32, 16, 0.25
    g = torch.Generator().manual_seed(groups + len(mode))
    wt, dy = draw((cout, cin, 3, 3), g, True), draw((n, cout, h, h), g, True)
    bnx = draw((n, cin, h, h), g, True)
    mean = torch.randint(-1, 2, (groups, cin), generator=g).double()
    coef = torch.stack([torch.tensor([0.5, 1.0, 2.0, -1.0])[torch.randint(0, 4, (cin,), generator=g)],
                        torch.randint(-1, 2, (cin,), generator=g).float() + 0.5]).contiguous()
    pre = bnx * coef[0].double()[None, :, None, None] + coef[1].double()[None, :, None, None]
    post = pre if mode == "post_coef" else draw((n, cin, h, h), g, True) + 0.5
    dxr = _grads64(torch.zeros(n, cin, h, h, dtype=torch.float64), wt, dy, 1, 0, "x")
    gg = dxr if mode == "neither" else torch.where(post > 0, dxr, dxr * slope)
    wd, dyd = wt.float().to(DEV), nhwc(dy).float().to(DEV)
    pk = O.PackSet()
    pk.add("x", "b", wd, h, h, cin, cout, dir=1)
    pk.finalize(dyd.device).run()
    nch = O.stat_chunks(n, h, h, cin, cout, 1, 0, groups, bwd=True)
    assert nch == n * h * h // 32
    part, pbuf = padded(nch * cin * 2, torch.float64)
    dx, dxbuf = padded(n * h * h * cin)
    dx.fill_(float("nan"))
    st = (part, groups, nhwc(bnx).float().to(DEV), nhwc(post).float().to(DEV) if mode == "post" else None,
          mean.float().to(DEV), slope) + (((coef.to(DEV), 0, 1),) if mode == "post_coef" else ())
    O.conv3x3_bwd_data(dyd, None, dx, n, h, h, cin, cout, wp=pk["b"], stats=st)
    ml = main_launch(O.last_launches())
    assert ml.kernel == "cgl_conv_fwd" and "STATS_BWD" in ml.flags
    torch.cuda.synchronize()
    canary_ok(pbuf, part.numel(), "st_part")
    canary_ok(dxbuf, dx.numel(), "dx")
    check(nchw(dx.view(n, h, h, cin)), dxr, None, True, "stats bwd dx", {})
    grow, xrow = nhwc(gg).reshape(-1, cin), nhwc(bnx).reshape(-1, cin)
    rows_per_call = n // groups * h * h
    got = part.view(nch, cin, 2).cpu()
    for ch in range(nch):
        blk = slice(ch * 32, ch * 32 + 32)
        mu = mean[ch * 32 // rows_per_call]
        assert torch.equal(got[ch, :, 0], grow[blk].sum(0)), f"chunk {ch}: sum g"
        assert torch.equal(got[ch, :, 1], (grow[blk] * (xrow[blk] - mu)).sum(0)), f"chunk {ch}: sum g (x - mean)"


# ---------------------------------------------------------------------------------------------------------------
# Dense ops (1 x 1 "convolutions" through the same dispatch): exact cases per route.
# (M, K, N, forward route, input-gradient route, weight-gradient kernel)
DENSE = [
    (37, 37, 70, "cgl_conv_fwd<1,1> 1x1x4", "cgl_conv_fwd<1,1> 1x1x4", "cgl_conv_wgrad"),       # K % 4 != 0: non-FAST
    (300, 64, 40, "cgl_conv_fwd<1,1,FAST> 1x1x4", "cgl_conv_fwd<1,1,FAST> 1x1x4", "cgl_conv_wgrad"),
    (64, 512, 1, "cgl_conv_n1", "cgl_conv_fwd<1,1> 1x1x4", "cgl_dense1_wgrad_k"),
    (7, 300, 1, "cgl_conv_fwd<1,1,FAST> 1x1x4", "cgl_conv_fwd<1,1> 1x1x4", "cgl_dense1_wgrad_k"),
]


@pytest.mark.parametrize("M,K,N,rf,rb,kw", DENSE)
def test_dense_routes_exact(M, K, N, rf, rb, kw):
    O = ops()
    g = torch.Generator().manual_seed(M + K + N)
    x, w, b, dy = draw((M, K), g, True), draw((N, K), g, True), draw((N,), g, True), draw((M, N), g, True)
    xd, wd, bd, dyd = x.float().to(DEV), w.float().to(DEV), b.float().to(DEV), dy.float().to(DEV)
    y, ybuf = padded(M * N)
    y.fill_(float("nan"))
    O.dense_fwd(xd, wd, bd, y, M, K, N, O.ACT_LEAKY, 0.25)
    assert route(main_launch(O.last_launches())) == rf
    pre = x @ w.t() + b
    check(y.view(M, N), torch.where(pre > 0, pre, pre * 0.25), None, True, "dense fwd", {})
    dx, dxbuf = padded(M * K)
    dx.fill_(float("nan"))
    O.dense_bwd_data(dyd, wd, dx, M, K, N)
    assert route(main_launch(O.last_launches())) == rb
    check(dx.view(M, K), dy @ w, None, True, "dense bwd_data", {})
    dw, dwbuf = padded(N * K)
    db, dbbuf = padded(N)
    dw.fill_(float("nan"))
    db.fill_(float("nan"))
    O.dense_bwd_weight(dyd, xd, dw, db, M, K, N)
    assert O.last_launches()[0].kernel == kw
    check(dw.view(N, K), dy.t() @ x, None, True, "dense bwd_weight", {})
    check(db, dy.sum(0), None, True, "dense bias grad", {})
    torch.cuda.synchronize()
    for t, bf, k in ((y, ybuf, "y"), (dx, dxbuf, "dx"), (dw, dwbuf, "dw"), (db, dbbuf, "db")):
        canary_ok(bf, t.numel(), "dense " + k)
