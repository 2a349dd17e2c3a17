"""ConvGanStep(colocated=W): one context with one G and W discriminators against W lockstep contexts
ConvGanStep(n_workers=W, rank=q) under ConvLocalComm -- same seeds, same initial state -- bitwise: parameters,
gradients, Adam moments, running statistics, loss words, alpha, the combined image gradient, lambda and every record
of the per-worker round logs; eager and graph rounds (run / run_rounds), bf16 operands, resume, the E-share of
ConvColocatedExchange and train_conv's lines.  And against oracle/conv_oracle.ConvCapgan with
test_gpu_conv_multiworker's rule: ||hip - fp64|| <= max(1e-5 ||fp64||, 4 ||fp32 - fp64||).  B = 8 throughout."""
import json

import pytest
import torch

from oracle import conv_oracle as CO

pytestmark = pytest.mark.gpu
B = 8
SHARDS = [20, 12, 9]     # ragged: every shard crosses a pass boundary within six rounds and has a short batch
BETA3 = [0.2, 0.3, 0.5]
PRE_BN_BIAS = {"conv_blocks.1.bias", "conv_blocks.5.bias"}
REC_FIELDS = ("round", "d_real", "d_fake", "d_loss", "g_loss", "alpha", "F", "lambda_", "real_rows", "g_step",
              "d_step")


def _shards(W, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(n, 1024, generator=g) * 2 - 1).cuda() for n in SHARDS[:W]]


def _beta(W):
    return BETA3 if W == 3 else [0.25, 0.75]


def _pair(W, weighting="capgan", shards=None, graph=False, gemm_dtype="f32", seed=7):
    from cglgan.conv_step import ConvGanStep
    from cglgan.exchange import ConvLocalComm
    beta = _beta(W)
    steps = []
    for r in range(W):
        s = ConvGanStep(B, loss="mse", seed=seed, n_workers=W, rank=r, weighting=weighting, beta=beta, graph=graph,
                        data=shards[r] if shards else None, gemm_dtype=gemm_dtype)
        s.init_default(20211212, 20211213 + r)
        steps.append(s)
    co = ConvGanStep(B, loss="mse", seed=seed, colocated=W, weighting=weighting, beta=beta, graph=graph, data=shards,
                     gemm_dtype=gemm_dtype)
    co.init_default(20211212, [20211213 + r for r in range(W)])
    return co, steps, ConvLocalComm(steps)


def _assert_same(co, steps, tag=""):
    torch.cuda.synchronize()
    g0 = steps[0].G
    for k in ("p", "g", "m", "v"):
        assert torch.equal(getattr(co.G, k), getattr(g0, k)), f"{tag} G.{k}"
    for k, v in g0.running.items():
        assert torch.equal(co.G.running[k], v), f"{tag} G {k}"
    assert co.G.batches == g0.batches and co.G.step == g0.step
    for q, s in enumerate(steps):
        d = co.Ds[q]
        for k in ("p", "g", "m", "v"):
            assert torch.equal(getattr(d, k), getattr(s.D, k)), f"{tag} D{q}.{k}"
        for k, v in s.D.running.items():
            assert torch.equal(d.running[k], v), f"{tag} D{q} {k}"
        assert d.batches == s.D.batches and d.step == s.D.step
        assert torch.equal(co.lbuf_all[q], s.lbuf), f"{tag} lbuf {q}"
        assert co.stats(worker=q)["g_loss"] == s.stats()["g_loss"]
    assert co.D is co.Ds[0]
    assert torch.equal(co.alpha_all, steps[0].alpha_all), f"{tag} alpha"
    assert torch.equal(co.losses_all, steps[0].losses_all), f"{tag} losses"
    assert torch.equal(co.dimg, steps[0].dimg), f"{tag} dimg"
    assert co.lam == steps[0].lam and co.round == steps[0].round
    assert float(co.rblk[0]) == float(steps[0].rblk[0]), f"{tag} device lambda"


def _assert_logs(co, steps, first, count):
    for q, s in enumerate(steps):
        a, b = co.read_log(first, count, worker=q), s.read_log(first, count)
        for i in range(count):
            for f in REC_FIELDS:
                assert getattr(a[i], f) == getattr(b[i], f), (q, first + i, f)


def _reals(W, g, short=None):
    out = []
    for q in range(W):
        n = B if short is None or short[q] is None else short[q]
        out.append((torch.rand(n, 1, 32, 32, generator=g) * 2 - 1).cuda())
    return out


@pytest.mark.parametrize("W,weighting", [(3, "capgan"), (2, "capgan"), (3, "mean")])
def test_eager_explicit_reals(W, weighting):
    co, steps, comm = _pair(W, weighting)
    g = torch.Generator().manual_seed(9)
    for rnd in range(2):
        reals = _reals(W, g, short=[None, 5, None][:W] if rnd == 1 else None)     # round 2: worker 1's batch short
        comm.round(rnd, reals=reals)
        co.run(reals=reals)
        _assert_same(co, steps, f"round {rnd + 1}")
    _assert_logs(co, steps, 1, 2)
    assert co.read_log(2, 1, worker=1)[0].real_rows == 5
    assert co.G.step == 2 and all(d.step == 2 for d in co.Ds)


@pytest.mark.parametrize("W", [3, 2])
def test_graph_rounds_ragged_shards(W):
    """Round 1 eager, one run() replay, then run_rounds(4): the state after round 6 and every record of rounds
    1 .. 6 of every worker against the lockstep contexts (their split-round graphs)."""
    shards = _shards(W)
    co, steps, comm = _pair(W, "capgan", shards=shards, graph=True)
    co.run()
    co.run()
    co.run_rounds(4)
    for rnd in range(6):
        comm.round(rnd)
    _assert_same(co, steps, "after round 6")
    _assert_logs(co, steps, 1, 6)
    rows = {q: [r.real_rows for r in co.read_log(1, 6, worker=q)] for q in range(W)}
    for q in range(W):
        assert SHARDS[q] % B in rows[q] and B in rows[q], rows      # short and whole batches were logged
    assert co._kgraphs and co._cuda_graph is not None               # the replays did run as graphs


def test_bf16_round():
    co, steps, comm = _pair(2, "capgan", gemm_dtype="bf16")
    reals = _reals(2, torch.Generator().manual_seed(4))
    comm.round(0, reals=reals)
    co.run(reals=reals)
    _assert_same(co, steps, "bf16")
    assert co.stats()["gemm_dtype"] == "bf16"


def _err(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).norm())


def _check(name, hip, o64, o32, fails, tol=1e-5):
    e = _err(hip, o64)
    bound = max(tol * float(o64.detach().double().norm()), 4 * _err(o32, o64), 1e-12)
    if e > bound:
        fails.append(f"{name}: err {e:.3e} > bound {bound:.3e}")


def _split(sd):
    return ({k: v.cpu() for k, v in sd.items() if "running" not in k and "num_batches" not in k},
            {k: v.cpu() for k, v in sd.items() if "running" in k or "num_batches" in k})


def test_oracle_three_workers():
    from cglgan.conv_step import ConvGanStep
    torch.set_num_threads(4)
    W = 3
    co = ConvGanStep(B, loss="mse", seed=7, colocated=W, weighting="capgan", beta=BETA3)
    co.init_default(20211212, [20211213 + r for r in range(W)])
    gp, gb = _split(co.G.state_dict())
    ds = [_split(d.state_dict()) for d in co.Ds]
    o64 = CO.ConvCapgan(gp, gb, [d[0] for d in ds], [d[1] for d in ds], BETA3, weighting="capgan",
                        dtype=torch.float64)
    o32 = CO.ConvCapgan(gp, gb, [d[0] for d in ds], [d[1] for d in ds], BETA3, weighting="capgan",
                        dtype=torch.float32)
    g = torch.Generator().manual_seed(9)
    for rnd in range(2):
        reals = [torch.rand(B, 1, 32, 32, generator=g) * 2 - 1 for _ in range(W)]
        co.run(reals=[x.cuda() for x in reals])
        torch.cuda.synchronize()
        z = co.z.cpu()
        masks = [([m[:B].cpu() for m in w["mask_d"]], [m[B:].cpu() for m in w["mask_d"]],
                  [m.cpu() for m in w["mask_g"]]) for w in co.workers]
        r64 = o64.round(z[:B], z[B:], reals, masks)
        r32 = o32.round(z[:B], z[B:], reals, masks)
        fails = []
        _check("losses", co.lbuf_all[:, 2].cpu(), r64["losses"], r32["losses"], fails)
        _check("Xg", co.xg().permute(0, 3, 1, 2), r64["Xg"], r32["Xg"], fails)
        for k, v in r64["g_grads"].items():
            if k not in PRE_BN_BIAS:
                _check(f"r{rnd} G grad {k}", co.G.grads[k], v, r32["g_grads"][k], fails)
        for i, d in enumerate(co.Ds):
            for k, v in r64["d_grads"][i].items():
                _check(f"r{rnd} D{i} grad {k}", d.grads[k], v, r32["d_grads"][i][k], fails)
            for k, v in d.params.items():
                _check(f"r{rnd} D{i} param {k}", v, o64.dps[i][k], o32.dps[i][k], fails)
        for k, v in co.G.params.items():
            if k not in PRE_BN_BIAS:
                _check(f"r{rnd} G param {k}", v, o64.gp[k], o32.gp[k], fails)
        assert not fails, "\n".join(fails)
        assert abs(co.lam - o64.lam) <= 1e-12


@pytest.mark.parametrize("graph", [False, True])
def test_resume(graph):
    from cglgan.conv_step import ConvGanStep
    W, shards = 2, _shards(2)

    def make():
        s = ConvGanStep(B, loss="mse", seed=5, colocated=W, weighting="capgan", beta=_beta(W), graph=graph,
                        data=shards)
        s.init_default(20211212, [20211213 + r for r in range(W)])
        return s
    whole = make()
    for _ in range(4):
        whole.run()
    a = make()
    a.run()
    a.run()
    sd = a.resume_state()
    b = make()
    b.init_default(1, 2)                    # another start: everything must come from the state
    b.load_resume_state(sd)
    with pytest.raises(LookupError):
        b.read_log(1, 1, worker=1)          # the rings were cleared
    b.run()
    b.run()
    torch.cuda.synchronize()
    assert b.round == whole.round == 4 and b.lam == whole.lam
    for k in ("p", "m", "v"):
        assert torch.equal(getattr(b.G, k), getattr(whole.G, k)), k
        for q in range(W):
            assert torch.equal(getattr(b.Ds[q], k), getattr(whole.Ds[q], k)), (q, k)
    for q in range(W):
        for k, v in whole.Ds[q].running.items():
            assert torch.equal(b.Ds[q].running[k], v), (q, k)
        assert b.Ds[q].step == 4 and b.Ds[q].batches == whole.Ds[q].batches
        assert b.losses_log(3, 2, worker=q) == whole.losses_log(3, 2, worker=q)


@pytest.mark.parametrize("graph", [False, True])
def test_e_share(graph):
    from cglgan.exchange import ConvColocatedExchange
    W = 2
    co, steps, comm = _pair(W, "capgan", shards=_shards(W), graph=graph)
    ex = ConvColocatedExchange(co, share_every=2)
    assert ex.chunks(0, 4) == [2, 2] and ex.chunks(1, 4) == [1, 2, 1] and ex.step is co
    ex.rounds(0, 4)
    for rnd in range(4):
        comm.round(rnd, share_every=2)
    _assert_same(co, steps, "after 4 rounds, 2 shares")
    assert torch.equal(co.Ds[0].p, co.Ds[1].p)                      # round 4 ended with a share
    for k, v in co.Ds[0].running.items():
        assert torch.equal(co.Ds[1].running[k], v)


def test_train_conv_lines():
    from cglgan.conv_driver import train_conv
    W = 2
    co, steps, comm = _pair(W, "capgan", shards=_shards(W), graph=True)
    lines = []
    lams = train_conv(co, 6, rounds_per_launch=4, log_every=1, log=lines.append)
    for rnd in range(6):
        comm.round(rnd)
    ref = steps[0].losses_log(1, 6)
    assert len(lines) == 6 and len(lams) == 6
    for ln, st in zip(map(json.loads, lines), ref):
        assert ln["round"] == st["round"] and ln["server"] == 0
        for k in ("d_loss", "g_loss", "lambda", "F"):
            assert ln[k] == st[k], (ln["round"], k)
    _assert_same(co, steps, "after train_conv")


def test_refusals():
    from cglgan.conv_step import ConvGanStep
    from cglgan.exchange import ConvColocatedExchange, ConvWorkerExchange
    shards = _shards(3)
    bad = [dict(colocated=1), dict(colocated=17), dict(colocated=3, n_workers=2), dict(colocated=3, rank=1),
           dict(colocated=3, data=shards[:2]), dict(colocated=3, data=shards[0]),
           dict(colocated=3, data=[t.cpu() for t in shards]), dict(colocated=3, data=[t.double() for t in shards]),
           dict(colocated=3, data=[shards[0], shards[1], shards[2][:, :1000]]),
           dict(colocated=3, data=shards, beta=[0.5, 0.5]), dict(colocated=3, data=shards, gemm_dtype="f16")]
    for kw in bad:
        with pytest.raises(ValueError):
            ConvGanStep(B, **kw)
    co = ConvGanStep(B, colocated=3, n_workers=3, data=shards)
    with pytest.raises(ValueError):
        ConvWorkerExchange(co)
    with pytest.raises(ValueError):
        co.run(real=shards[0][:B])
    with pytest.raises(ValueError):
        co.run(reals=[shards[0][:B]])
    with pytest.raises(ValueError):
        co.stats(worker=3)
    with pytest.raises(ValueError):
        co.set_beta([1.0])
    one = ConvGanStep(B)
    with pytest.raises(ValueError):
        ConvColocatedExchange(one)
    with pytest.raises(ValueError):
        one.run(reals=[shards[0][:B]])
    with pytest.raises(ValueError):
        one.read_log(1, 1, worker=1)
