"""The conv GAN round with bf16 MFMA operands (ConvGanStep(gemm_dtype="bf16")).

The reference has no 16-bit arithmetic, so a whole bf16 round's parity is UNPINNED; the design follows
tests/test_gpu_lowp.py and uses no fixed error number.  From one initial state, seed, real batch and the Dropout2d
masks read back from the device, oracle.conv_oracle.ConvGan runs twice in fp64:
  * ``exact``: as it is;
  * ``emu``: with ``conv_oracle.F`` replaced (here, not in oracle/) by a proxy of torch.nn.functional whose conv2d
    is a custom autograd function -- forward on bf16-rounded input and weight; backward rounds dY and calls
    torch.nn.grad.conv2d_input / conv2d_weight on the rounded operands; bias gradient from the unrounded dY -- for
    every conv the HIP path runs on MFMA kernels (Conv2d(64, 1), Conv2d(1, 16) and both Linears stay unrounded).
    ``emu`` is only approximate: it rounds each 3x3 tap where the device rounds the phase-combined taps.
e(t) = ||emu - exact|| measures the bf16 error of tensor t from the reference alone.  Required, for the losses, Xd,
Xg and every G / D gradient (the pre-BatchNorm biases' gradients are analytically zero: exempt):
    ||hip - exact|| <= 3 e(t)
(3 covers two independent roundings of equal size (sqrt 2), the combined-tap difference and neighbour flips; a wrong
fragment layout or k order is O(1) relative, tens of times e), and for Xg
    ||hip_bf16 - hip_fp32|| >= 0.1 e(Xg)
so that a step that never engaged the mode fails.  The fp32 step must itself be within 0.1 e(t) of ``exact`` on
every judged tensor (asserted: the comparison is not vacuous).
"""
import os

import pytest
import torch
import torch.nn.functional as TF

from oracle import conv_oracle as CO

pytestmark = pytest.mark.gpu
PRE_BN_BIAS = {"conv_blocks.1.bias", "conv_blocks.5.bias"}   # gradient == 0 analytically


def _rb(t):
    return t.float().bfloat16().to(t.dtype)


class _Bf16Conv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, stride, padding):
        xr, wr = _rb(x), _rb(w)
        ctx.save_for_backward(xr, wr)
        ctx.geo = (stride, padding, b is not None)
        return TF.conv2d(xr, wr, b, stride, padding)

    @staticmethod
    def backward(ctx, dy):
        xr, wr = ctx.saved_tensors
        stride, padding, has_b = ctx.geo
        dyr = _rb(dy)
        dx = torch.nn.grad.conv2d_input(xr.shape, wr, dyr, stride, padding)
        dw = torch.nn.grad.conv2d_weight(xr, wr.shape, dyr, stride, padding)
        db = dy.sum(dim=(0, 2, 3)) if has_b else None
        return dx, dw, db, None, None


class _FProxy:
    """torch.nn.functional with conv2d rounded as the MFMA kernels round (vector-kernel layers untouched)."""

    def __getattr__(self, name):
        return getattr(TF, name)

    @staticmethod
    def conv2d(x, w, b=None, stride=1, padding=0):
        if w.shape[0] == 1 or w.shape[1] == 1:      # Conv2d(64, 1), Conv2d(1, 16): vector-ALU kernels, fp32
            return TF.conv2d(x, w, b, stride, padding)
        return _Bf16Conv.apply(x, w, b, stride, padding)


def _norm(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).norm())


# The seed.  e(t) of a scalar loss is a SIGNED sum of the 8 samples' errors, and at some seeds it cancels to nearly
# nothing: e(d_fake) over seeds 1 .. 8 is 6.5e-8, 9.8e-9, 2.9e-9, 2.4e-8, 2.2e-7, 9.0e-8, 9.6e-8, 1.2e-9 (median
# 4.5e-8), where the HIP round's own d_fake error stays near 1e-7 at every seed -- so at seeds 3 and 8 "3 e" asks for
# 30 to 150 times less than the bf16 error of that loss (measured: 28 e and 145 e there, <= 1.2 e on every tensor).
# The seed is therefore picked from the REFERENCE ALONE (emu and exact, no HIP figure): of seeds 1 .. 8 the one whose
# three loss yardsticks e(d_real), e(d_fake), e(g_loss) are all closest to typical -- the largest minimum of
# e(loss) / median over the seeds of e(loss): seed 7 (0.94; the others 0.77, 0.22, 0.06, 0.54, 0.28, 0.73, 0.03).
# Measured on the MI355X at seed 7: worst judged quantity 1.43 e (losses 0.99 / 0.79 / 1.32 e), the fp32 step at
# most 0.003 e; at seed 3 every tensor-valued quantity (Xd, Xg, all gradients) was 0.3 .. 1.2 e.
SEED = 7


def _parity_round(seed, B=8):
    """One round of the bf16 step, the fp32 step and the two fp64 oracle runs from one state, seed and inputs."""
    from cglgan.conv_step import ConvGanStep
    n_thr = torch.get_num_threads()
    torch.set_num_threads(4)
    steps = {}
    for dt in ("bf16", "f32"):
        st = ConvGanStep(B, loss="mse", seed=seed, gemm_dtype=dt)
        st.init_default(20211212, 20211213)
        steps[dt] = st
    st = steps["bf16"]
    split = lambda sd: ({k: v.cpu() for k, v in sd.items() if "running" not in k and "num_batches" not in k},
                        {k: v.cpu() for k, v in sd.items() if "running" in k or "num_batches" in k})
    gp, gb = split(st.G.state_dict())
    dp, db = split(st.D.state_dict())
    exact = CO.ConvGan(gp, gb, dp, db, loss="mse", dtype=torch.float64)
    emu = CO.ConvGan(gp, gb, dp, db, loss="mse", dtype=torch.float64)
    real = torch.rand(B, 1, 32, 32, generator=torch.Generator().manual_seed(seed)) * 2 - 1
    for s in steps.values():
        s.run(real=real.cuda())
    torch.cuda.synchronize()
    z = st.z.cpu()
    assert torch.equal(z, steps["f32"].z.cpu())
    mr, mf = [m[:B].cpu() for m in st.mask_d], [m[B:].cpu() for m in st.mask_d]
    mg = [m.cpu() for m in st.mask_g]
    assert all(torch.equal(a, b) for a, b in zip(st.mask_d + st.mask_g, steps["f32"].mask_d + steps["f32"].mask_g))
    rx = exact.round(z[:B], z[B:], real, mr, mf, mg)
    old = CO.F
    CO.F = _FProxy()
    try:
        re = emu.round(z[:B], z[B:], real, mr, mf, mg)
    finally:
        CO.F = old
    torch.set_num_threads(n_thr)

    def tensors(s):
        sd = s.stats()
        out = {k: torch.tensor(sd[k], dtype=torch.float64) for k in ("d_real", "d_fake", "g_loss")}
        out["Xd"], out["Xg"] = s.xd().permute(0, 3, 1, 2), s.xg().permute(0, 3, 1, 2)
        out.update({"G grad " + k: v for k, v in s.G.grads.items() if k not in PRE_BN_BIAS})
        out.update({"D grad " + k: v for k, v in s.D.grads.items()})
        return out

    def oracle(r):
        out = {k: torch.tensor(r[k], dtype=torch.float64) for k in ("d_real", "d_fake", "g_loss")}
        out["Xd"], out["Xg"] = r["Xd"], r["Xg"]
        out.update({"G grad " + k: v for k, v in r["g_grads"].items() if k not in PRE_BN_BIAS})
        out.update({"D grad " + k: v for k, v in r["d_grads"].items()})
        return out
    return tensors(steps["bf16"]), tensors(steps["f32"]), oracle(rx), oracle(re), steps


@pytest.fixture(scope="module")
def parity():
    """Shared by the tests below (computed once)."""
    return _parity_round(SEED)


def test_bf16_round_within_the_references_own_bf16_error(parity):
    hip, hip32, exact, emu, steps = parity
    assert steps["bf16"].stats()["gemm_dtype"] == "bf16" and steps["f32"].stats()["gemm_dtype"] == "f32"
    assert set(hip) == set(exact) == set(emu)
    fails = []
    for k in exact:
        e = _norm(emu[k], exact[k])
        d16, d32 = _norm(hip[k], exact[k]), _norm(hip32[k], exact[k])
        print(f"{k}: e {e:.3e}  |hip_bf16 - exact| {d16:.3e} ({d16 / max(e, 1e-300):.2f} e)  "
              f"|hip_fp32 - exact| {d32:.3e} ({d32 / max(e, 1e-300):.4f} e)")
        if not d32 <= 0.1 * e:
            fails.append(f"{k}: the fp32 step is {d32:.3e} from exact, above 0.1 e = {0.1 * e:.3e} (vacuous)")
        if not d16 <= 3 * e:
            fails.append(f"{k}: |hip - exact| {d16:.3e} > 3 e = {3 * e:.3e}")
    assert not fails, "\n".join(fails)


def test_bf16_round_engaged_the_mode(parity):
    hip, hip32, exact, emu, _ = parity
    e = _norm(emu["Xg"], exact["Xg"])
    d = _norm(hip["Xg"], hip32["Xg"])
    print(f"Xg: |hip_bf16 - hip_fp32| {d:.3e}, e {e:.3e}")
    assert e > 0 and d >= 0.1 * e


def test_f16_is_refused():
    from cglgan.conv_step import ConvGanStep
    with pytest.raises(ValueError, match="loss scaling"):
        ConvGanStep(8, gemm_dtype="f16")


def _data(B, seed, rows=None):
    return torch.rand(rows or 4 * B + 3, 1024, device="cuda", generator=torch.Generator("cuda").manual_seed(seed)) * 2 - 1


def _same_state(a, b):
    for name in ("p", "g", "m", "v"):
        assert torch.equal(getattr(a.G, name), getattr(b.G, name)), ("G", name)
        assert torch.equal(getattr(a.D, name), getattr(b.D, name)), ("D", name)
    for k in a.G.running:
        assert torch.equal(a.G.running[k], b.G.running[k]), k
    for k in a.D.running:
        assert torch.equal(a.D.running[k], b.D.running[k]), k
    assert torch.equal(a.lbuf, b.lbuf) and torch.equal(a.x3, b.x3)


def test_bf16_graph_replay_is_the_eager_round():
    from cglgan import conv_ops as O
    from cglgan.conv_step import ConvGanStep
    B = 8
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        data = _data(B, 3)
        a = ConvGanStep(B, seed=21, data=data, graph=True, gemm_dtype="bf16")
        b = ConvGanStep(B, seed=21, data=data, graph=True, gemm_dtype="bf16")
        a.init_default(5, 6)
        b.init_default(5, 6)
        for r in range(3):
            a.run(eager=True)
            b.run()              # round 0 eager, round 1 captured + replayed, round 2 a replay
        torch.cuda.synchronize()
    assert b._cuda_graph is not None and O.get_mma_dtype() == 0
    _same_state(a, b)


def test_bf16_multi_round_graph():
    from cglgan.conv_step import ConvGanStep
    B = 8
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        data = _data(B, 7, rows=3 * B + 5)
        a = ConvGanStep(B, seed=23, data=data, graph=True, gemm_dtype="bf16")
        b = ConvGanStep(B, seed=23, data=data, graph=True, gemm_dtype="bf16")
        a.init_default(8, 9)
        b.init_default(8, 9)
        a.run()
        b.run()
        a.run_rounds(3)
        for _ in range(3):
            b.run()
        torch.cuda.synchronize()
    assert set(a._kgraphs) == {3} and a.round == b.round == 4
    _same_state(a, b)
    assert torch.equal(a.dstate, b.dstate)


@pytest.mark.parametrize("var", ["CGL_CONV_HALO", "CGL_CONV_LDSM"])
def test_bf16_round_path_equivalences_bitwise(var):
    """B = 256, two eager bf16 rounds: the halo / LDS-panel kernels against the direct path (the form of
    test_conv_round_halo_bitwise) -- reaches the halo, LDSM and cgl_conv_wgrad_lds kernels inside a round."""
    from cglgan.conv_step import ConvGanStep
    B = 256
    data = _data(B, 3)
    steps = []
    for env in ("1", "0"):
        st = ConvGanStep(B, seed=21, data=data, graph=False, gemm_dtype="bf16")
        st.init_default(5, 6)
        os.environ[var] = env
        try:
            for _ in range(2):
                st.run(eager=True)
            torch.cuda.synchronize()
        finally:
            os.environ.pop(var, None)
        steps.append(st)
    a, b = steps
    _same_state(a, b)
    assert torch.equal(a.y2, b.y2)


def test_fp32_step_after_a_bf16_step_is_unchanged():
    from cglgan import conv_ops as O
    from cglgan.conv_step import ConvGanStep
    B = 8
    data = _data(B, 3)

    def run(dt):
        st = ConvGanStep(B, seed=21, data=data, graph=False, gemm_dtype=dt)
        st.init_default(5, 6)
        for _ in range(2):
            st.run()
        torch.cuda.synchronize()
        return st
    alone = run("f32")
    mid = run("bf16")
    assert O.get_mma_dtype() == 0
    after = run("f32")
    _same_state(alone, after)
    assert not torch.equal(alone.G.p, mid.G.p)


def test_bf16_two_workers_local_comm():
    from cglgan.conv_step import ConvGanStep
    from cglgan.exchange import ConvLocalComm
    N, B = 2, 8
    steps = []
    for r in range(N):
        g = torch.Generator().manual_seed(40 + r)
        data = (torch.rand(3 * B + 5, 1024, generator=g) * 2 - 1).cuda()
        s = ConvGanStep(B, loss="mse", seed=11, n_workers=N, rank=r, weighting="capgan", data=data, graph=True,
                        gemm_dtype="bf16")
        s.init_default(20211212, 20211213 + r)
        steps.append(s)
    comm = ConvLocalComm(steps)
    for r in range(2):
        comm.round(r, share_every=2)
    torch.cuda.synchronize()
    for s in steps:
        assert s.round == 2
        for t in (s.G.p, s.D.p, s.G.g, s.D.g, s.lbuf):
            assert bool(torch.isfinite(t).all())
    assert torch.equal(steps[0].G.p, steps[1].G.p)      # replicated G
