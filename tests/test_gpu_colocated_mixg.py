"""The co-located Mix-G / CGLGAN step (GanStep(specs.mixgen_group(W) | specs.ring_group(W), d, colocated=W,
exchange_layer=head layer)): one context holds the server's whole MixGenerator -- the trunk run once, the W heads and
the W discriminators as W-grouped launches, the hidden-layer gradient exchange inside the round
(mixed-gan.py:238-292 + :355-392, CGLGAN/2DMG/main.py:225-278 + :344-375).

  * against the reference-pinned oracle (MixgServer with mix_single / mix_double, CglganServer on the 2-D ring), with
    the method and bounds of test_gpu_configs.test_mixg_double_softmax_weighting and of the ring round tests;
  * bitwise against the lockstep form it replaces: W mixgen_worker(h) contexts under LocalComm;
  * multi-round graphs and the per-worker round logs; the plan's shape; state dicts and resume; the Cloud average.
"""
import copy
import types

import pytest
import torch

from cglgan import GanStep, specs
from cglgan.exchange import LocalComm, local_cloud_average
from cglgan.init import mixgen_state
from oracle import gan_oracle as O
from parity_helpers import STEP_TOL, TRAJ_TOL, lambda_within, masked_pair, rel_scalar, to_double, within
from test_gpu_cglgan_modules import _ring_inputs
from test_gpu_colocated_step import _d_flops
from test_gpu_configs import _check_d, _check_g, _round64w, _traj

pytestmark = pytest.mark.gpu

XL = specs.MIXGEN_HEAD_LAYER
# launches a co-located Mix-G round has beyond the one-worker Mix-G fp32 plan's: the round prologue stays a launch of
# its own (the one-worker plan folds it into G's first GEMM) and the local exchange adds cgl_alpha_combine
EXTRA_LAUNCHES = 2


@pytest.fixture(autouse=True)
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(8)
    yield
    torch.set_num_threads(n)


def _worker_masks(step, w):
    """parity_helpers.gpu_masks for worker w of a co-located step (cgl_gan_tensor code + 256 w: the trunk's layers
    shared, the head's layers and the D-side tensors the worker's own)."""
    gm, dm, B, Br = step.gm, step.dm, step.B, step.Br
    o = 256 * w
    gt = [step.internal(o + ((48 + l) if gm.bn[l] else (64 + l))).view(2 * B, -1) > 0 for l in range(gm.n_layers - 1)]
    P = [step.internal(o + 112 + j).view(Br + B, -1) > 0 for j in range(dm.n_layers - 1)]
    S = [step.internal(o + 128 + j).view(B, -1) > 0 for j in range(dm.n_layers - 1)]
    return {"g": [[t[:B].cpu() for t in gt], [t[B:].cpu() for t in gt]],
            "d": [[p[:Br].cpu() for p in P], [p[Br:].cpu() for p in P], [s.cpu() for s in S]]}


def _as_workers(co):
    """The co-located step seen as its W workers, for the helpers that take one step per worker."""
    return [types.SimpleNamespace(d_views=co.d_views[w], stats=(lambda w=w: co.stats(worker=w)))
            for w in range(co.colocated)]


def _feed(co, z1, z2, reals):
    B = co.B
    co.z[:B].copy_(z1)
    co.z[B:].copy_(z2)
    for w, r in enumerate(reals):
        co.real[w].copy_(r.reshape(r.shape[0], -1))


# ------------------------------------------------------------------------------------------------ 1. oracle, Mix-G
@pytest.mark.parametrize("N,beta,weighting", [(3, [0.2, 0.3, 0.5], "mix_single"), (2, [0.3, 0.7], "mix_double")],
                         ids=["mix_single_3", "mix_double_2"])
def test_oracle_parity_mixg(N, beta, weighting):
    """Two rounds (the second with lambda > 0) against MixgServer, with the method and the bounds of
    test_gpu_configs.test_mixg_double_softmax_weighting; the default plan (every fusion as planned)."""
    B = 64
    g_sd, d_sds = mixgen_state(N, n_discriminators=N)
    G, workers = O.build_mixg(N)
    srv = O.MixgServer(G, torch.tensor(beta), weighting=weighting)
    co = GanStep(specs.mixgen_group(N), specs.mnist_discriminator(), batch=B, colocated=N, weighting=weighting,
                 exchange_layer=XL)
    co.load_state_dicts(g_sd, d_sds)
    co.reset(beta=beta)
    srv64, workers64 = copy.deepcopy(srv), copy.deepcopy(workers)
    to_double(srv64, workers64)

    def inputs(seed):
        z1, z2, reals = O.synthetic_inputs(B, N, 1, seed=seed)
        return z1, z2, [rs[0] for rs in reals]

    z1, z2, reals = inputs(61)
    _feed(co, z1, z2, reals)
    co.run()
    torch.cuda.synchronize()
    masks = [_worker_masks(co, w) for w in range(N)]
    _, m64 = masked_pair(srv.G, workers, srv64.G, workers64, masks, head_layer=XL)
    srv.round(workers, z1, z2, [[x] for x in reals])
    _round64w(srv64, workers64, z1, z2, [[x] for x in reals])
    m64.check_signs()
    fails = _check_g(co, srv.G, srv64.G, list(co.g_views))          # the trunk and every head
    assert not fails, fails
    assert len(co.g_views) == 10 + 6 * N
    assert not _check_d(_as_workers(co), workers, workers64)
    # a second round with lambda > 0
    z1, z2, reals = inputs(1061)
    _feed(co, z1, z2, reals)
    co.run()
    torch.cuda.synchronize()
    masks = [_worker_masks(co, w) for w in range(N)]
    m32, m64 = masked_pair(srv.G, workers, srv64.G, workers64, masks, head_layer=XL)
    out = srv.round(workers, z1, z2, [[x] for x in reals])
    _round64w(srv64, workers64, z1, z2, [[x] for x in reals])
    m64.check_signs()
    m32.check_signs()
    _traj(_as_workers(co), out, "round 2")
    st = co.stats()
    assert st["round"] == 2 and float(out["lam"]) > 0
    assert rel_scalar(st["F"], out["F"]) <= TRAJ_TOL and abs(st["lambda"] - float(out["lam"])) <= 1e-7


# ------------------------------------------------------------------------------------------------ 2. oracle, ring
def test_oracle_parity_cglgan_ring():
    """CGLGAN/2DMG (no BatchNorm, a 32-wide exchange tensor, a 2-wide output) against CglganServer: every tensor
    within parity_helpers.within, lambda within the cancellation bound of parity_helpers.lambda_within."""
    N, B = 2, 64
    G, workers = O.build_ring(N, N)
    srv = O.CglganServer(G, torch.full((N,), 1.0 / N))
    co = GanStep(specs.ring_group(N), specs.ring_discriminator(), batch=B, loss="bce", weighting="cglgan",
                 colocated=N, exchange_layer=specs.RING_HEAD_LAYER)
    co.load_state_dicts(G.state_dict(), [w.D.state_dict() for w in workers])
    co.reset()
    srv64, workers64 = copy.deepcopy(srv), copy.deepcopy(workers)
    to_double(srv64, workers64)
    z1, z2, reals = _ring_inputs(srv, workers, B, 31)
    _feed(co, z1, z2, reals)
    co.run()
    torch.cuda.synchronize()
    r32 = srv.round(workers, z1, z2, [[r] for r in reals])
    r64 = _round64w(srv64, workers64, z1, z2, [[r] for r in reals])
    sts = [co.stats(worker=w) for w in range(N)]
    fails = []
    got = {"d_losses": torch.tensor([s["d_loss"][0] for s in sts]), "g_losses": torch.tensor([s["g_loss"] for s in sts]),
           "F": torch.tensor([sts[0]["F"]])}
    for key, v in got.items():
        ok, e, a = within(v, r32[key].reshape(-1), r64[key].reshape(-1), tol=STEP_TOL)
        if not ok:
            fails.append((key, e, a))
    ok, e, a = lambda_within(sts[0]["lambda"], got["g_losses"], r64["lam"], r64["g_losses"])
    if not ok:
        fails.append(("lam", e, a))
    g32 = {k: v for n in [srv.G.trunk] + list(srv.G.heads) for k, v in n.params.items()}
    g64 = {k: v for n in [srv64.G.trunk] + list(srv64.G.heads) for k, v in n.params.items()}
    assert list(co.g_views) == list(g32)
    for k, p in co.g_views.items():
        gr = co.g_grad_views[k]
        gd = gr.detach().double().cpu().flatten() - g64[k].grad.detach().double().flatten()
        ok, e, a = within(gr, g32[k].grad, g64[k].grad)
        if not ok:
            fails.append(("G grad", k, e, a))
        extra = 1.5 * float((2e-4 * gd.abs() / (g64[k].grad.detach().double().flatten().abs() + 1e-8)).norm())
        ok, e, a = within(p, g32[k], g64[k], extra)
        if not ok:
            fails.append(("G param", k, e, a))
    for i in range(N):
        for k, p in co.d_views[i].items():
            q32, q64 = workers[i].D.params[k], workers64[i].D.params[k]
            gd = co.d_grad_views[i][k].detach().double().cpu().flatten() - q64.grad.detach().double().flatten()
            extra = 1.5 * float((2e-4 * gd.abs() / (q64.grad.detach().double().flatten().abs() + 1e-8)).norm())
            ok, e, a = within(p, q32, q64, extra)
            if not ok:
                fails.append(("D param", i, k, e, a))
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ 3. bitwise
def _pair(ring=False, W=3, B=64, Br=None, epoch=1, gemm_dtype="f32", weighting=None, seed=5, state_seed=20211212):
    """(lockstep contexts, co-located step) from the same initial state and the same caller-supplied inputs."""
    if ring:
        group, dm, img, xl = specs.ring_group(W), specs.ring_discriminator(), 2, specs.RING_HEAD_LAYER
        G, workers = O.build_ring(W, W, seed=state_seed)
        g_sd, d_sds = G.state_dict(), [w.D.state_dict() for w in workers]
        kw = dict(loss="bce", weighting=weighting or "cglgan")
    else:
        group, dm, img, xl = specs.mixgen_group(W), specs.mnist_discriminator(), 784, XL
        g_sd, d_sds = mixgen_state(W, seed=state_seed, n_discriminators=W)
        kw = dict(loss="ce", weighting=weighting or "mix_single")
    kw.update(batch=B, batch_real=Br, epoch=epoch, gemm_dtype=gemm_dtype, exchange_layer=xl)
    beta = [0.2, 0.3, 0.5] if W == 3 else None
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(2 * B, 100, generator=gen)
    reals = torch.rand(W, epoch * (Br or B), img, generator=gen) * 2 - 1
    steps = []
    for h in range(W):
        s = GanStep(group.head_spec(h), dm, n_workers=W, rank=h, **kw)
        s.load_state_dicts(g_sd, d_sds[h])
        s.reset(beta=beta)
        s.z.copy_(z)
        s.real.copy_(reals[h])
        steps.append(s)
    co = GanStep(group, dm, colocated=W, **kw)
    co.load_state_dicts(g_sd, d_sds)
    co.reset(beta=beta)
    co.z.copy_(z)
    co.real.copy_(reals)
    return steps, co


def _flat(step, buf, key):
    """The slice of a flat G buffer (g_grads, g_m, g_v, ...) that holds tensor `key`."""
    v = step.g_views[key]
    o = v.storage_offset() - step.g_params.storage_offset()
    return buf[o:o + v.numel()]


def _assert_same_group(steps, co):
    torch.cuda.synchronize()
    trunk = [k for k in co.g_views if k.startswith("model.")]
    assert trunk and len(co.g_views) == len(trunk) + len(steps) * (len(steps[0].g_views) - len(trunk))
    for w, s in enumerate(steps):
        own = [k for k in co.g_views if k.startswith(f"paths.{w}.")]
        assert sorted(trunk + own) == sorted(s.g_views)
        for k in trunk + own:               # the trunk against every context's, head w against context w's
            for name in ("g_params", "g_grads", "g_m", "g_v"):
                assert torch.equal(_flat(co, getattr(co, name), k), _flat(s, getattr(s, name), k)), (w, k, name)
        for k, v in s.running.items():      # the trunk's and head w's running statistics
            assert torch.equal(co.running[k], v), (w, k)
        assert torch.equal(co.d_params[w], s.d_params), w
        assert torch.equal(co.d_grads[w], s.d_grads), w
        assert torch.equal(co.d_m[w], s.d_m) and torch.equal(co.d_v[w], s.d_v), w
        assert torch.equal(co.exchange_buffer(), s.exchange_buffer()), w
        a, b = co.stats(worker=w), s.stats()
        for k in ("round", "d_loss", "d_real", "d_fake", "g_loss", "alpha", "F", "lambda"):
            assert a[k] == b[k], (w, k, a[k], b[k])


@pytest.mark.parametrize("kw,rounds", [
    (dict(), 2),                    # two rounds: the second reads the packed copies the first round's launches wrote
    (dict(Br=40), 1),               # a worker's last head workgroup is partial
    (dict(epoch=2), 1),             # two local D steps per round
    (dict(gemm_dtype="bf16"), 1),   # 16-bit GEMM operands
    (dict(W=16, B=16), 1),          # the cap on co-located workers
    (dict(ring=True, W=2), 1),      # no BatchNorm, tiny widths, the cglgan weighting
], ids=["mix_single_3", "batch_real_40", "epoch_2", "bf16", "cap_16_workers", "ring_cglgan_2"])
def test_bitwise_against_lockstep(kw, rounds):
    """One round (two in the base case) of W mixgen_worker(h) contexts under LocalComm and of the co-located step,
    from the same state and inputs: every tensor and scalar equal bit for bit.  Both sides run their default plans:
    the fusions the co-located plan leaves off (the prologue folded into G's first GEMM, the deferred loss-head
    reduction, the packing jobs carried by head-side launches) change no GEMM's tile choice, so no environment
    switch is needed on either side."""
    steps, co = _pair(**kw)
    lc = LocalComm(steps)
    for r in range(rounds):
        lc.round(r)
        co.run()
    _assert_same_group(steps, co)


# ------------------------------------------------------------------------------------------------ 4. graphs, logs
def _sampled(W=3, B=64, seed=77):
    g_sd, d_sds = mixgen_state(W, n_discriminators=W)
    real = torch.rand(320, 784, generator=torch.Generator().manual_seed(3)).cuda() * 2 - 1
    shards = [(0, 150), (150, 100), (250, 70)]
    s = GanStep(specs.mixgen_group(W), specs.mnist_discriminator(), batch=B, colocated=W, weighting="mix_single",
                exchange_layer=XL, gen_z=True, real=real, sample_n=150, shards=shards, seed=seed)
    s.load_state_dicts(g_sd, d_sds)
    s.reset(beta=[0.5, 0.3, 0.2])
    return s


_REC_FIELDS = ("round", "d_loss", "d_real", "d_fake", "g_loss", "alpha", "F", "lambda", "real_rows", "loss_scale",
               "step_skipped")


def test_multi_round_graph_and_log():
    """run_rounds(4) (one graph of four rounds) against four single run() calls: the state bitwise, every worker's
    log records field by field."""
    a, b = _sampled(), _sampled()
    a.run_rounds(4)
    for _ in range(4):
        b.run()
    torch.cuda.synchronize()
    for k in GanStep._RESUME_BUFS + ("g_grads", "d_grads"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert torch.equal(a.internal(6).view(torch.int32), b.internal(6).view(torch.int32))
    for w in range(3):
        ra, rb = a.losses_log(1, 4, worker=w), b.losses_log(1, 4, worker=w)
        assert [r["round"] for r in ra] == [1, 2, 3, 4]
        for x, y in zip(ra, rb):
            for f in _REC_FIELDS:
                assert x[f] == y[f], (w, x["round"], f, x[f], y[f])
        assert ra[-1]["g_loss"] == a.stats(worker=w)["g_loss"] and ra[-1]["alpha"] == a.stats(worker=w)["alpha"]
    # the shards of 100 and 70 rows end their passes with short batches, the workers' losses differ
    assert a.losses_log(2, 1, worker=1)[0]["real_rows"] == [36] and a.losses_log(2, 1, worker=2)[0]["real_rows"] == [6]
    assert len({a.losses_log(4, 1, worker=w)[0]["g_loss"] for w in range(3)}) == 3


# ------------------------------------------------------------------------------------------------ 5. plan
def _g_flops(m, B, lo, hi):
    """GEMM FLOPs of G layers [lo, hi): the forward over 2B rows, the weight gradient and (layers >= 1) the input
    gradient over B rows."""
    return sum(2.0 * m.dims[l] * m.dims[l + 1] * (2 * B + B + (B if l >= 1 else 0)) for l in range(lo, hi))


def test_plan_shape():
    dm, B = specs.mnist_discriminator(), 64
    kw = dict(batch=B, weighting="mix_single", exchange_layer=XL)
    one = GanStep(specs.mixgen_worker(0), dm, **kw)
    two = GanStep(specs.mixgen_group(2), dm, colocated=2, **kw)
    four = GanStep(specs.mixgen_group(4), dm, colocated=4, **kw)
    n1, n2, n4 = len(one.launches()), len(two.launches()), len(four.launches())
    assert n2 == n4 == n1 + EXTRA_LAUNCHES
    k2, k4 = [k for k, _, _ in two.launches()], [k for k, _, _ in four.launches()]
    assert k2 == k4 and k2.count("alpha_combine") == 1 and k2.count("prologue") == 1
    assert sum(g for _, _, g in four.launches()) > sum(g for _, _, g in two.launches())
    m = specs.mixgen_worker(0)
    trunk, head = _g_flops(m, B, 0, XL), _g_flops(m, B, XL, m.n_layers)
    for W, s in ((2, two), (4, four)):
        assert s.plan_info()["gemm_flops"] == trunk + W * (head + _d_flops(B, B, 1))
    # the ring: two layers, no BatchNorm launches at all
    ring = [GanStep(specs.ring_group(W), specs.ring_discriminator(), batch=B, loss="bce", weighting="cglgan",
                    colocated=W, exchange_layer=specs.RING_HEAD_LAYER) for W in (2, 4)]
    assert len(ring[0].launches()) == len(ring[1].launches())
    assert not any(k.startswith("bn") for k, _, _ in ring[0].launches())


# ------------------------------------------------------------------------------------------------ 6. state, resume
def test_state_dicts_and_resume():
    from cglgan.model import MixGenerator
    W = 3
    a = _sampled()
    a.run_rounds(2)
    sd = a.g_state_dict()
    net = MixGenerator((1, 28, 28), W)
    net.load_state_dict(sd, strict=True)                      # every key of the module, none beside them
    assert int(net.paths[2][1].num_batches_tracked) == 4
    b = _sampled()
    b.load_state_dicts(net.state_dict(), [a.d_state_dict(w) for w in range(W)])
    torch.cuda.synchronize()
    assert torch.equal(a.g_params, b.g_params) and torch.equal(a.g_running, b.g_running)
    assert torch.equal(a.d_params, b.d_params)
    # resume: two more rounds from the saved state in a fresh step, bitwise
    rs = a.resume_state()
    a.run_rounds(2)
    c = _sampled()
    c.load_resume_state(rs)
    with pytest.raises(LookupError):
        c.read_log(1, 2, worker=1)
    c.run_rounds(2)
    torch.cuda.synchronize()
    for k in GanStep._RESUME_BUFS:
        assert torch.equal(getattr(a, k), getattr(c, k)), k
    for w in range(W):
        ra, rc = a.losses_log(3, 2, worker=w), c.losses_log(3, 2, worker=w)
        assert ra == rc and [r["round"] for r in rc] == [3, 4]
    assert a.stats(worker=2) == c.stats(worker=2)


# ------------------------------------------------------------------------------------------------ 7. Cloud
def test_cloud_average_of_two_servers():
    """Two servers of two workers: one round each, the Cloud average of the trunks (parameters and running
    statistics, weights A), a second round.  The lockstep side takes the same average -- sum_s A_s trunk_s over one
    context per server, in server order -- and every context of a server continues from it; the heads are not
    touched by the average."""
    S, H = 2, 2
    A = [0.4, 0.6]
    pairs = [_pair(W=H, seed=11 + s, state_seed=20211212 + s) for s in range(S)]
    comms = [LocalComm(steps) for steps, _ in pairs]
    for (steps, co), lc in zip(pairs, comms):
        lc.round(0)
        co.run()
    local_cloud_average([co for _, co in pairs], A, cloud_scope="trunk")
    local_cloud_average([steps[0] for steps, _ in pairs], A, cloud_scope="trunk")
    for steps, _ in pairs:
        p0, r0 = steps[0].trunk_slices()
        for s in steps[1:]:
            p, r = s.trunk_slices()
            p.copy_(p0)
            r.copy_(r0)
    torch.cuda.synchronize()
    t0 = pairs[0][1].trunk_slices()
    for steps, co in pairs:
        p, r = co.trunk_slices()
        assert torch.equal(p, t0[0]) and torch.equal(r, t0[1])            # one trunk on both servers
        assert p.numel() == steps[0].trunk_slices()[0].numel() and r.numel() == steps[0].trunk_slices()[1].numel()
        for w, s in enumerate(steps):
            assert torch.equal(p, s.trunk_slices()[0]) and torch.equal(r, s.trunk_slices()[1]), w
            for k in s.g_views:
                assert torch.equal(co.g_views[k], s.g_views[k]), (w, k)  # the averaged trunk, the untouched head
    assert not torch.equal(pairs[0][1].g_views["paths.0.0.weight"], pairs[1][1].g_views["paths.0.0.weight"])
    for (steps, co), lc in zip(pairs, comms):       # the packed copies follow the average: the next round agrees
        lc.round(1)
        co.run()
        _assert_same_group(steps, co)
