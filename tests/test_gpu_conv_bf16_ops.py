"""bf16 MFMA operands of the conv ops (cgl_conv_set_mma_dtype, conv_ops.mma_dtype): every kernel path of the four
MFMA families, op by op.

The mode rounds fp32 operands this test supplies, as they enter the MFMA, and accumulates in fp32.  Products of two
bf16 values are exact in fp32, so the mode is emulated exactly -- up to fp32 accumulation order -- by the FP32 MODE OF
THE SAME ENTRY POINT fed operands rounded at the same point:
  * X and dY rounded with ``t.bfloat16().float()``;
  * the weights as the fp32 packed operand of a PackSet, rounded the same way and passed through ``wp=`` ("combine
    the phase taps in fp32, then round", without restating the phase algebra);
  * weight gradients from the rounded dY and the rounded X; the bias gradient from the rounded dY where it rides the
    im2col ones-column, from the unrounded dY where cgl_conv3x3_bias_by_colsum reports the column-sum path;
  * the folded-BatchNorm (bn_in) forms against the unfolded path: the activation cgl_eltwise wrote (bitwise the
    folded arithmetic), rounded, through the plain fp32 conv.
Non-upsampled cases are also checked against torch's fp64 conv2d and its autograd on the rounded operands (no
weight combination there).

Tolerance: the conv ops' own bound, 2e-5 x the reference's max magnitude (``close`` of test_gpu_conv_ops).  A kernel
that misses a rounding, or rounds before the BatchNorm / the phase combination, is off by ~4e-3 per operand.
How the 16-bit MFMA sums inside a chunk had not been measured before.  Observed on the MI355X (``_close`` prints
every figure): the largest error of any case is 1.0e-6 x max|ref| (the LDSM input gradient), 5e-7 .. 9e-7 for the
up-convolutions' forwards and ~1e-7 elsewhere; the ones-column bias gradients are bitwise the reference's.  The plain
bound holds 20-fold, so the per-element sum-bound widening the design would allow is not used: no excess to record.
"""
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
REL = 2e-5


def ops():
    from cglgan import conv_ops
    return conv_ops


def rb(t):
    """Round to bf16 (nearest even) and back: the value the MFMA sees."""
    return t.bfloat16().float()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _close(got, ref, what):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    scale = max(float(ref.abs().max()), 1e-12)
    err = float((got - ref).abs().max())
    print(f"{what}: max err {err:.3e}, scale {scale:.3e}, ratio {err / scale:.3e} (bound {REL:.0e})")
    assert err <= REL * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def _env(name, val, fn):
    os.environ[name] = val
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    finally:
        os.environ.pop(name, None)


def _packed(w, h, wd, cin, cout, stride, up):
    """The fp32 packed forward / input-gradient operands of ``w`` (phase taps combined in fp32)."""
    O = ops()
    pk = O.PackSet()
    pk.add("L", "f", w, h, wd, cin, cout, stride, up)
    pk.add("L", "b", w, h, wd, cin, cout, stride, up, dir=1)
    pk.finalize(w.device)
    pk.run()
    torch.cuda.synchronize()
    return pk["f"].clone(), pk["b"].clone()


def _operands(n, h, w, cin, cout, stride, up, seed):
    O = ops()
    g = torch.Generator(DEV).manual_seed(seed)
    ho, wo = O.conv_out_hw(h, w, stride, up)
    x = torch.randn(n, h, w, cin, device=DEV, generator=g)
    wt = torch.randn(cout, cin, 3, 3, device=DEV, generator=g) / (3 * cin ** 0.5)
    b = torch.randn(cout, device=DEV, generator=g) * 0.1
    dy = torch.randn(n, ho, wo, cout, device=DEV, generator=g)
    return x, wt, b, dy, ho, wo


MMA_CASES = [
    # n, h, w, cin, cout, stride, up
    (3, 16, 16, 16, 32, 2, 0),      # direct path, in-workgroup split-K
    (2, 4, 4, 64, 128, 2, 0),
    (2, 7, 7, 32, 64, 2, 0),        # odd sizes, ragged tiles
    (2, 9, 7, 32, 48, 1, 0),        # stride 1, ragged tiles in M and N
    (1, 5, 3, 16, 16, 1, 1),        # phase-form upsampling outside the halo path
    (2, 16, 16, 128, 64, 1, 1),     # halo forward
    (3, 8, 8, 128, 128, 1, 1),      # halo forward, two 64-channel workgroups per row tile
    (16, 8, 8, 128, 128, 1, 1),     # cgl_conv_wgrad_lds, WM = 2
    (8, 16, 16, 128, 64, 1, 1),     # cgl_conv_wgrad_lds, WM = 1
    (32, 8, 8, 128, 128, 1, 0),     # cgl_conv_wgrad_lds, 9 direct taps
]


@pytest.mark.parametrize("n,h,w,cin,cout,stride,up", MMA_CASES)
def test_bf16_conv_fwd_bwd(n, h, w, cin, cout, stride, up):
    O = ops()
    geo = (n, h, w, cin, cout, stride, up)
    x, wt, b, dy, ho, wo = _operands(*geo, seed=n * 1000 + h * 10 + cin + cout)
    wpf, wpb = _packed(wt, h, w, cin, cout, stride, up)
    xr, dyr = rb(x), rb(dy)
    e = lambda *s: torch.empty(*s, device=DEV)
    # ---- forward: plain and packed entry points in bf16 mode vs the fp32 mode on rounded operands
    with O.mma_dtype("bf16"):
        y = O.conv3x3_fwd(x, wt, b, e(n, ho, wo, cout), *geo, O.ACT_LEAKY, 0.2).clone()
        yp = O.conv3x3_fwd(x, wt, b, e(n, ho, wo, cout), *geo, O.ACT_LEAKY, 0.2, wp=wpf).clone()
        dx = O.conv3x3_bwd_data(dy, wt, e(n, h, w, cin), *geo).clone()
        dxp = O.conv3x3_bwd_data(dy, wt, e(n, h, w, cin), *geo, wp=wpb).clone()
        dw, db = e(cout, cin, 3, 3), e(cout)
        O.conv3x3_bwd_weight(dy, x, dw, db, *geo)
    assert O.get_mma_dtype() == 0
    y_ref = O.conv3x3_fwd(xr, wt, b, e(n, ho, wo, cout), *geo, O.ACT_LEAKY, 0.2, wp=rb(wpf))
    _close(y, y_ref, "fwd")
    assert torch.equal(y, yp), "fwd: the packed entry point differs from the packing one"
    dx_ref = O.conv3x3_bwd_data(dyr, wt, e(n, h, w, cin), *geo, wp=rb(wpb))
    _close(dx, dx_ref, "bwd_data")
    assert torch.equal(dx, dxp), "bwd_data: the packed entry point differs from the packing one"
    dw_ref, db_r = e(cout, cin, 3, 3), e(cout)
    O.conv3x3_bwd_weight(dyr, xr, dw_ref, db_r, *geo)
    _close(dw, dw_ref, "bwd_weight")
    if ops().C.lib.cgl_conv3x3_bias_by_colsum(*geo) == 1:
        db_u = e(cout)
        O.conv3x3_bwd_weight(dy, x, e(cout, cin, 3, 3), db_u, *geo)
        assert torch.equal(db, db_u), "bias grad: the column-sum path must stay the fp32 sum of the unrounded dY"
    else:
        _close(db, db_r, "bias grad (ones-column: sum of the rounded dY)")
    # ---- independent: torch fp64 on the rounded operands (no weight combination without upsampling)
    if not up:
        x64 = nchw(xr).double().cpu().requires_grad_(True)
        w64 = rb(wt).double().cpu().requires_grad_(True)
        y64 = F.conv2d(x64, w64, b.double().cpu(), stride, 1)
        _close(nchw(y), F.leaky_relu(y64, 0.2), "fwd vs fp64")
        y64.backward(nchw(dyr).double().cpu())
        _close(nchw(dx), x64.grad, "bwd_data vs fp64")
        _close(dw, w64.grad, "bwd_weight vs fp64")


def test_bf16_ldsm_input_gradient():
    """The LDS-panel path (128 x 128 tiles, 2 x 2 waves): only reached at the benchmarked size, the input gradient
    of Upsample + Conv2d(128, 64) over 256 images.  GPU reference only; CGL_CONV_LDSM=0 is bitwise equal."""
    O = ops()
    n, geo = 256, (256, 16, 16, 128, 64, 1, 1)
    g = torch.Generator(DEV).manual_seed(1)
    dy = torch.randn(n, 32, 32, 64, device=DEV, generator=g)
    wt = torch.randn(64, 128, 3, 3, device=DEV, generator=g) / 30
    _, wpb = _packed(wt, 16, 16, 128, 64, 1, 1)
    run = lambda d, wp: O.conv3x3_bwd_data(d, wt, torch.empty(n, 16, 16, 128, device=DEV), *geo, wp=wp)
    with O.mma_dtype("bf16"):
        a = _env("CGL_CONV_LDSM", "1", lambda: run(dy, wpb))
        b = _env("CGL_CONV_LDSM", "0", lambda: run(dy, wpb))
    assert torch.equal(a, b)
    ref = _env("CGL_CONV_LDSM", "1", lambda: run(rb(dy), rb(wpb)))
    _close(a, ref, "ldsm bwd_data")
    assert not torch.equal(a, run(dy, wpb)), "the bf16 mode changed nothing"


def test_bf16_halo_bitwise():
    """CGL_CONV_HALO=1 vs 0 in bf16 mode at test_upconv_halo_op_bitwise's smallest size: the same fragment values
    and one MFMA per chunk in the same order."""
    O = ops()
    n, hw, cout = 128, 16, 64
    g = torch.Generator(DEV).manual_seed(7)
    x = torch.randn(n, hw, hw, 128, device=DEV, generator=g)
    wt = torch.randn(cout, 128, 3, 3, device=DEV, generator=g) * 0.05
    b = torch.randn(cout, device=DEV, generator=g)
    run = lambda: O.conv3x3_fwd(x, wt, b, torch.empty(n, 2 * hw, 2 * hw, cout, device=DEV), n, hw, hw, 128, cout, 1,
                                1, O.ACT_LEAKY, 0.2)
    with O.mma_dtype("bf16"):
        a = _env("CGL_CONV_HALO", "1", run)
        c = _env("CGL_CONV_HALO", "0", run)
    assert torch.equal(a, c)
    assert not torch.equal(a, run()), "the bf16 mode changed nothing"


def _bn_producer(n, h, w, cin, cout, stride, up, groups, act, seed):
    """A conv with epilogue statistics and the BatchNorm finalize that keeps scale / shift: returns the pre-BatchNorm
    map y, the activation a = act(BN(y)) written by cgl_eltwise, and coef [2][groups][cout]."""
    O = ops()
    x, wt, b, _, ho, wo = _operands(n, h, w, cin, cout, stride, up, seed)
    wpf, _ = _packed(wt, h, w, cin, cout, stride, up)
    nch = O.stat_chunks(n, h, w, cin, cout, stride, up, groups)
    assert nch > 0
    part = torch.zeros(nch * cout * 2, dtype=torch.float64, device=DEV)
    y = torch.empty(n, ho, wo, cout, device=DEV)
    O.conv3x3_fwd(x, wt, b, y, n, h, w, cin, cout, stride, up, wp=wpf, stats=(part, groups))
    g = torch.Generator(DEV).manual_seed(seed + 1)
    gamma = torch.rand(cout, device=DEV, generator=g) + 0.5
    beta = torch.randn(cout, device=DEV, generator=g) * 0.3
    a = torch.empty_like(y)
    coef = torch.zeros(2 * groups * cout, device=DEV)
    O.bn2d_fwd_stats(part, y, n, ho * wo, cout, gamma, beta, a, groups=groups, act=act, slope=0.2,
                     scratch=O.bn2d_stats_scratch(cout, groups, DEV), coef=coef, apply_from=0)
    torch.cuda.synchronize()
    return y, a, coef


BNIN_CASES = [
    # producer geometry, groups, activation; consumer geometry (the round's B = 8 shapes)
    ((16, 8, 8, 128, 128, 1, 1), 2, 1, (16, 16, 16, 128, 64, 1, 1)),    # G conv_blocks.5 (halo, folded BatchNorm)
    ((8, 16, 16, 16, 32, 2, 0), 1, 0, (8, 8, 8, 32, 64, 2, 0)),          # D model.4's BatchNorm into Conv2d(32, 64)
    ((8, 8, 8, 32, 64, 2, 0), 1, 0, (8, 4, 4, 64, 128, 2, 0)),           # D model.8's BatchNorm into Conv2d(64, 128)
]


@pytest.mark.parametrize("prod,groups,act,cons", BNIN_CASES)
def test_bf16_folded_batchnorm_forward(prod, groups, act, cons):
    O = ops()
    y, a, coef = _bn_producer(*prod, groups, act, seed=sum(prod))
    n, h, w, cin, cout, stride, up = cons
    x2, wt, b, _, ho, wo = _operands(*cons, seed=sum(cons))
    wpf, _ = _packed(wt, h, w, cin, cout, stride, up)
    out = lambda: torch.empty(n, ho, wo, cout, device=DEV)
    with O.mma_dtype("bf16"):
        got = O.conv3x3_fwd(y, wt, b, out(), *cons, O.ACT_LEAKY, 0.2, wp=wpf, bn_in=(coef, groups, act, 0.2)).clone()
    ref = O.conv3x3_fwd(rb(a), wt, b, out(), *cons, O.ACT_LEAKY, 0.2, wp=rb(wpf))
    _close(got, ref, "bnin fwd")
    # rounding before the BatchNorm instead of after it is far outside the bound: the reference must tell them apart
    early = O.conv3x3_fwd(rb(y), wt, b, out(), *cons, O.ACT_LEAKY, 0.2, wp=rb(wpf), bn_in=(coef, groups, act, 0.2))
    assert float((early - ref).abs().max()) > 10 * REL * float(ref.abs().max())


@pytest.mark.parametrize("prod,groups,group,act,cons", [
    ((16, 8, 8, 128, 128, 1, 1), 2, 1, 1, (8, 16, 16, 128, 64, 1, 1)),    # G conv_blocks.5: the LDS-staged kernel
    ((16, 16, 16, 16, 32, 2, 0), 2, -1, 0, (16, 8, 8, 32, 64, 2, 0)),     # D step: the wave-unit kernel, two calls
])
def test_bf16_bwd_weight_bnin(prod, groups, group, act, cons):
    O = ops()
    y, a, coef = _bn_producer(*prod, groups, act, seed=sum(prod) + 3)
    n, h, w, cin, cout, stride, up = cons
    if group >= 0:      # one forward call's images
        per = prod[0] // groups
        y, a = y[group * per:(group + 1) * per].contiguous(), a[group * per:(group + 1) * per].contiguous()
    ho, wo = O.conv_out_hw(h, w, stride, up)
    dy = torch.randn(n, ho, wo, cout, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    e = lambda *s: torch.empty(*s, device=DEV)
    dw, db = e(cout, cin, 3, 3), e(cout)
    with O.mma_dtype("bf16"):
        O.conv3x3_bwd_weight(dy, y, dw, db, *cons, bn_in=(coef, group, groups, act, 0.2))
    dw_ref, db_r = e(cout, cin, 3, 3), e(cout)
    O.conv3x3_bwd_weight(rb(dy), rb(a), dw_ref, db_r, *cons)
    _close(dw, dw_ref, "bnin bwd_weight")
    if O.C.lib.cgl_conv3x3_bias_by_colsum(*cons) == 1:
        db_u = e(cout)
        O.conv3x3_bwd_weight(dy, a, e(cout, cin, 3, 3), db_u, *cons)
        assert torch.equal(db, db_u)
    else:
        _close(db, db_r, "bnin bias grad")


@pytest.mark.parametrize("geo", [(2, 32, 32, 64, 1, 1, 0), (3, 32, 32, 1, 16, 2, 0)])
def test_vector_kernels_ignore_the_mode(geo):
    """Conv2d(64, 1) and Conv2d(1, 16): vector-ALU kernels in every direction, bitwise the fp32 results."""
    O = ops()
    n, h, w, cin, cout, stride, up = geo
    x, wt, b, dy, ho, wo = _operands(*geo, seed=11)
    e = lambda *s: torch.empty(*s, device=DEV)

    def run():
        y = O.conv3x3_fwd(x, wt, b, e(n, ho, wo, cout), *geo, O.ACT_LEAKY, 0.2)
        dx = O.conv3x3_bwd_data(dy, wt, e(n, h, w, cin), *geo)
        dw, db = e(cout, cin, 3, 3), e(cout)
        O.conv3x3_bwd_weight(dy, x, dw, db, *geo)
        torch.cuda.synchronize()
        return y, dx, dw, db
    ref = run()
    with O.mma_dtype("bf16"):
        got = run()
    for name, p, q in zip(("fwd", "bwd_data", "bwd_weight", "bias grad"), got, ref):
        assert torch.equal(p, q), name


def test_dense_ignores_the_mode():
    O = ops()
    M, K, N = 64, 512, 1
    g = torch.Generator(DEV).manual_seed(2)
    x = torch.randn(M, K, device=DEV, generator=g)
    w = torch.randn(N, K, device=DEV, generator=g) / K ** 0.5
    b = torch.randn(N, device=DEV, generator=g)
    ref = O.dense_fwd(x, w, b, torch.empty(M, N, device=DEV), M, K, N).clone()
    with O.mma_dtype("bf16"):
        got = O.dense_fwd(x, w, b, torch.empty(M, N, device=DEV), M, K, N).clone()
    assert torch.equal(got, ref)
    # an MFMA-routed dense layer (N > 1) stays fp32 as well
    M, K, N = 37, 100, 70
    x = torch.randn(M, K, device=DEV, generator=g)
    w = torch.randn(N, K, device=DEV, generator=g) / K ** 0.5
    b = torch.randn(N, device=DEV, generator=g)
    ref = O.dense_fwd(x, w, b, torch.empty(M, N, device=DEV), M, K, N).clone()
    with O.mma_dtype("bf16"):
        got = O.dense_fwd(x, w, b, torch.empty(M, N, device=DEV), M, K, N).clone()
    assert torch.equal(got, ref)


def test_mode_does_not_leak():
    O = ops()
    geo = (2, 9, 7, 32, 48, 1, 0)
    n, h, w, cin, cout, stride, up = geo
    x, wt, b, _, ho, wo = _operands(*geo, seed=4)
    run = lambda: O.conv3x3_fwd(x, wt, b, torch.empty(n, ho, wo, cout, device=DEV), *geo).clone()
    first = run()
    with O.mma_dtype("bf16"):
        mid = run()
    third = run()
    assert torch.equal(first, third)
    assert not torch.equal(first, mid)
    assert O.get_mma_dtype() == 0
