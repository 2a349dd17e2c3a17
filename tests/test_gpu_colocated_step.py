"""The co-located step (GanStep(colocated=W)): one context runs the W-worker CAPGAN / MD-GAN round of a server
group (capgan.py:211-262 + :316-349) -- G once, every D stage one launch over the W workers.

  * against the reference-pinned oracle (oracle.gan_oracle.CapganServer.round), with the inputs, seed search and
    bounds of test_gpu_multiworker.test_capgan_three_workers_beta_weighted;
  * bitwise against the lockstep path it replaces: W one-worker-per-context GanSteps under LocalComm;
  * the plan: launches independent of W, within a constant of the one-worker plan, FLOPs = G + W * D;
  * resume.
"""
import copy

import pytest
import torch

from cglgan import GanStep, specs
from cglgan.exchange import LocalComm
from cglgan.init import topology_state
from oracle import gan_oracle as O
from parity_helpers import to_double, within
from test_gpu_multiworker import _check_params, _round64, _seed_ok

pytestmark = pytest.mark.gpu

# launches a co-located round may have beyond the one-worker plan's: the round prologue stays a launch of its own
# (the one-worker fp32 plan folds it into G's first GEMM) and the local exchange adds cgl_alpha_combine
EXTRA_LAUNCHES = 2


@pytest.fixture(autouse=True)
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def test_oracle_parity_three_workers_beta_weighted():
    N, B = 3, 64
    beta = [0.2, 0.3, 0.5]
    G, workers = O.build_capgan(N)
    srv = O.CapganServer(G, torch.tensor(beta))
    step = GanStep(specs.mnist_generator(), specs.mnist_discriminator(), batch=B, colocated=N)
    step.load_state_dicts(G.state_dict(), [w.D.state_dict() for w in workers])
    step.reset(beta=beta)
    srv64, workers64 = copy.deepcopy(srv), copy.deepcopy(workers)
    to_double(srv64, workers64)
    for seed in range(40, 104):
        z1, z2, reals = O.synthetic_inputs(B, N, 1, seed=seed)
        if _seed_ok(G, workers, z1, z2, reals):
            break
    step.z[:B].copy_(z1)
    step.z[B:].copy_(z2)
    for r in range(N):
        step.real[r].copy_(reals[r][0])
    step.run()
    torch.cuda.synchronize()
    r32 = srv.round(workers, z1, z2, reals)
    r64 = _round64(srv64, workers64, z1, z2, reals)
    st = step.stats()
    assert abs(st["F"] - float(r64["F"])) <= max(1e-5 * abs(float(r64["F"])), 2 * abs(float(r32["F"] - r64["F"])))
    assert abs(st["lambda"] - float(r32["lam"])) <= 1e-7
    fails = _check_params(step, srv.G, srv64.G, list(step.g_views))
    assert not fails, fails
    for r in range(N):
        for k, v in step.d_views[r].items():
            ok, e, a = within(v, workers[r].D.params[k], workers64[r].D.params[k])
            assert ok, (r, k, e, a)


def _pair(W=3, B=64, Br=None, epoch=1, mdgan=False, gemm_dtype="f32", seed=5):
    """(lockstep contexts, co-located step) from the same initial state and the same caller-supplied inputs."""
    gm = specs.mnist_generator()
    dm = specs.mnist_discriminator(sigmoid=mdgan)
    gs, ds = topology_state("mdgan" if mdgan else "capgan", 1, W, 20211212, 784)
    kw = dict(batch=B, batch_real=Br, epoch=epoch, loss="bce" if mdgan else "ce",
              weighting="mean" if mdgan else "capgan", gemm_dtype=gemm_dtype)
    beta = [0.2, 0.3, 0.5][:W] if W == 3 else None
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(2 * B, 100, generator=gen)
    reals = torch.rand(W, epoch * (Br or B), 784, generator=gen) * 2 - 1
    steps = []
    for r in range(W):
        s = GanStep(gm, dm, n_workers=W, rank=r, **kw)
        s.load_state_dicts(gs[0], ds[r])
        s.reset(beta=beta)
        s.z.copy_(z)
        s.real.copy_(reals[r])
        steps.append(s)
    co = GanStep(gm, dm, colocated=W, **kw)
    co.load_state_dicts(gs[0], ds)
    co.reset(beta=beta)
    co.z.copy_(z)
    co.real.copy_(reals)
    return steps, co


def _assert_same_round(steps, co):
    torch.cuda.synchronize()
    for w, s in enumerate(steps):
        assert torch.equal(co.g_params, s.g_params), w
        assert torch.equal(co.d_params[w], s.d_params), w
        assert torch.equal(co.d_grads[w], s.d_grads), w
        assert torch.equal(co.d_m[w], s.d_m) and torch.equal(co.d_v[w], s.d_v), w
        a, b = co.stats(worker=w), s.stats()
        for k in ("round", "d_loss", "d_real", "d_fake", "g_loss", "alpha", "F", "lambda"):
            assert a[k] == b[k], (w, k, a[k], b[k])
    assert torch.equal(co.g_grads, steps[0].g_grads)
    assert torch.equal(co.g_running, steps[0].g_running)
    assert torch.equal(co.exchange_buffer(), steps[0].exchange_buffer())


@pytest.mark.parametrize("kw", [
    dict(),
    dict(Br=40),                    # the head's last workgroup of a worker is partial
    dict(epoch=2),
    dict(mdgan=True),               # BCE, weighting "mean", sigmoid D
    dict(gemm_dtype="bf16"),
    dict(W=16, B=16),               # the cap on co-located workers
], ids=["capgan", "batch_real_40", "epoch_2", "mdgan", "bf16", "cap_16_workers"])
def test_bitwise_against_lockstep(kw):
    steps, co = _pair(**kw)
    LocalComm(steps).round(0)
    co.run()
    _assert_same_round(steps, co)


def test_second_round_and_two_workers():
    """Two rounds (the packed D copies the first round's grouped Adam wrote are what the second reads), W = 2."""
    steps, co = _pair(W=2)
    lc = LocalComm(steps)
    for r in range(2):
        lc.round(r)
        co.run()
    _assert_same_round(steps, co)


def _d_flops(B, Br, epoch):
    """GEMM FLOPs of one worker's D work in a round, from the layer sizes: per local step the hidden forwards, every
    layer's weight gradient and the hidden input gradients over Br + B rows; the G-loss pass's hidden forwards and
    input gradients (down to the image) over B rows.  (The output layer's forward and input gradient are the loss
    head's, not GEMMs.)"""
    d = specs.mnist_discriminator().dims
    J, Md = len(d) - 1, Br + B
    hid = sum(d[j] * d[j + 1] for j in range(J - 1))
    every = sum(d[j] * d[j + 1] for j in range(J))
    igrad = sum(d[j] * d[j + 1] for j in range(1, J - 1))
    return epoch * 2.0 * Md * (hid + every + igrad) + 2.0 * B * (hid + hid)


def test_grouping_launches_and_flops(monkeypatch):
    gm, dm = specs.mnist_generator(), specs.mnist_discriminator()
    B = 64
    one = GanStep(gm, dm, batch=B)
    # plan_info sums the plain GEMM launches: the one-worker plan's figure is taken with G's first GEMM as one of
    # them (not folded into the prologue launch), as it is in the co-located plan
    monkeypatch.setenv("CGL_FUSE_PRO", "0")
    one_flops = GanStep(gm, dm, batch=B).plan_info()["gemm_flops"]
    monkeypatch.delenv("CGL_FUSE_PRO")
    two = GanStep(gm, dm, batch=B, colocated=2)
    four = GanStep(gm, dm, batch=B, colocated=4)
    n1, n2, n4 = len(one.launches()), len(two.launches()), len(four.launches())
    assert n2 == n4
    assert n1 <= n2 <= n1 + EXTRA_LAUNCHES
    f1, f2, f4 = one_flops, two.plan_info()["gemm_flops"], four.plan_info()["gemm_flops"]
    dpart = f2 - f1                      # the second worker's D: what a worker adds to the plan
    assert dpart == _d_flops(B, B, 1)
    assert f4 == f1 + 3 * dpart
    # grouped, not repeated: the W = 4 plan has the W = 2 plan's launch kinds in the same order, larger grids
    k2, k4 = [k for k, _, _ in two.launches()], [k for k, _, _ in four.launches()]
    assert k2 == k4
    assert sum(g for _, _, g in four.launches()) > sum(g for _, _, g in two.launches())
    # with two local steps the count grows by one local step's launches, for any W
    e1 = GanStep(gm, dm, batch=B, epoch=2)
    e4 = GanStep(gm, dm, batch=B, epoch=2, colocated=4)
    assert len(e4.launches()) - n4 == len(e1.launches()) - n1


def test_resume():
    W, B = 3, 64
    gm, dm = specs.mnist_generator(), specs.mnist_discriminator()
    gs, ds = topology_state("capgan", 1, W, 20211212, 784)
    real = torch.rand(320, 784, generator=torch.Generator().manual_seed(3)).cuda() * 2 - 1
    shards = [(0, 150), (150, 100), (250, 70)]

    def make():
        s = GanStep(gm, dm, batch=B, colocated=W, gen_z=True, real=real, sample_n=150, shards=shards, seed=77)
        s.load_state_dicts(gs[0], ds)
        s.reset(beta=[0.5, 0.3, 0.2])
        return s

    a = make()
    a.run_rounds(2)
    sd = a.resume_state()
    a.run_rounds(2)
    b = make()
    b.load_resume_state(sd)
    with pytest.raises(LookupError):
        b.read_log(1, 2, worker=1)          # the old timeline's records are gone
    b.run_rounds(2)
    torch.cuda.synchronize()
    for k in GanStep._RESUME_BUFS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    for w in range(W):
        ra, rb = a.losses_log(3, 2, worker=w), b.losses_log(3, 2, worker=w)
        assert ra == rb and [r["round"] for r in rb] == [3, 4]
    assert a.stats(worker=2) == b.stats(worker=2)
