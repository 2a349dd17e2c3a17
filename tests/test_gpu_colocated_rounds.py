"""The co-located step over several rounds: the device sampler over unequal shards inside a K-round graph, the
D exchange object (E-share, MD-GAN D-swap) and the driver's ``colocate`` mode -- each bitwise against the lockstep
path (one GanStep context per worker under cglgan.exchange.LocalComm) on the same shards, seed and initial state."""
import json

import pytest
import torch

from cglgan import GanStep, specs
from cglgan._lib import GanRoundRec
from cglgan.exchange import ColocatedExchange, LocalComm
from cglgan.init import topology_state

pytestmark = pytest.mark.gpu

W, B = 3, 64
SHARDS = [(0, 150), (150, 100), (250, 70)]     # every worker meets a short batch and a new pass within 4 rounds
BETA = [150 / 320, 100 / 320, 70 / 320]


def _real():
    return (torch.rand(320, 784, generator=torch.Generator().manual_seed(9)) * 2 - 1).cuda()


def _build(mdgan=False, seed=4242):
    gm, dm = specs.mnist_generator(), specs.mnist_discriminator(sigmoid=mdgan)
    gs, ds = topology_state("mdgan" if mdgan else "capgan", 1, W, 20211212, 784)
    kw = dict(batch=B, loss="bce" if mdgan else "ce", weighting="mean" if mdgan else "capgan", gen_z=True, seed=seed)
    real = _real()
    steps = []
    for r, (a, n) in enumerate(SHARDS):
        s = GanStep(gm, dm, n_workers=W, rank=r, real=real[a:a + n], sample_n=n, **kw)
        s.load_state_dicts(gs[0], ds[r])
        s.reset(beta=BETA)
        steps.append(s)
    co = GanStep(gm, dm, colocated=W, real=real, sample_n=150, shards=SHARDS, **kw)
    co.load_state_dicts(gs[0], ds)
    co.reset(beta=BETA)
    return steps, co


def _assert_same_state(steps, co):
    torch.cuda.synchronize()
    for w, s in enumerate(steps):
        for k in ("g_params", "g_m", "g_v", "g_running"):
            assert torch.equal(getattr(co, k), getattr(s, k)), (w, k)
        for k in ("d_params", "d_m", "d_v", "d_grads"):
            assert torch.equal(getattr(co, k)[w], getattr(s, k)), (w, k)


def test_sampler_and_four_round_graph():
    steps, co = _build()
    lc = LocalComm(steps)
    for r in range(4):
        lc.round(r, graph=True)
    co.run_rounds(4)
    _assert_same_state(steps, co)
    short = set()
    for w, s in enumerate(steps):
        mine, ref = co.read_log(1, 4, worker=w), s.read_log(1, 4)
        for a, b in zip(mine, ref):
            for name, _ in GanRoundRec._fields_:
                va, vb = getattr(a, name), getattr(b, name)
                if hasattr(va, "__len__"):
                    va, vb = list(va), list(vb)
                assert va == vb, (w, b.round, name, va, vb)
            short.add((w, a.real_rows[0]))
    # the case the shards were chosen for: every worker had a full and a short batch
    assert short == {(0, 64), (0, 22), (1, 64), (1, 36), (2, 64), (2, 6)}
    assert co.stats()["round"] == 4


def test_exchange_object_share_and_swap():
    steps, co = _build(mdgan=True)
    lc = LocalComm(steps, share_every=2, swap_every=3)
    perms = [lc.round(r, graph=True) for r in range(6)]
    ex = ColocatedExchange(co, share_every=2, swap_every=3)
    assert ex.chunks(0, 4) == [2, 1, 1] and ex.chunks(4, 2) == [2]      # rounds_per_launch = 4: really cut
    ex.rounds(0, 4)
    ex.rounds(4, 2)
    _assert_same_state(steps, co)
    assert [p for p in perms if p is not None] and co.stats()["round"] == 6
    for w, s in enumerate(steps):
        assert co.losses_log(1, 6, worker=w) == s.losses_log(1, 6)


def test_exchange_round_by_round_matches_rounds():
    _, a = _build()
    _, b = _build()
    ea, eb = ColocatedExchange(a, share_every=2, swap_every=3), ColocatedExchange(b, share_every=2, swap_every=3)
    ea.rounds(0, 6)
    for r in range(6):
        eb.round(r)
    torch.cuda.synchronize()
    assert torch.equal(a.d_params, b.d_params) and torch.equal(a.g_params, b.g_params)


def test_driver_colocate_matches_lockstep():
    from cglgan.data import beta_weights
    from cglgan.driver import Driver, DriverConfig, Topology, gpu_step, make_shards

    # (num_sample: the test-sample draw of allocate_dataset must fit in the 600-row dataset; the default is 1000)
    kw = dict(num_workers=3, batch_size=64, dataset_rows=600, num_communication=6, rounds_per_launch=3, log_every=1,
              num_sample=100)
    cfg = DriverConfig(colocate=True, **kw)
    lines = []
    drv = Driver(cfg, rank=0, world=1)
    drv.run(log=lines.append)
    assert len(lines) == 6

    plain = DriverConfig(**kw)
    with pytest.raises(ValueError, match="one process per worker"):
        Driver(plain, rank=0, world=1)
    x, shards = make_shards(plain)
    beta, _ = beta_weights([len(s) for s in shards])
    gs, ds = topology_state("capgan", 1, 3, plain.seed, plain.img_size ** 2)
    dev = torch.device("cuda", torch.cuda.current_device())
    steps = [gpu_step(plain, Topology(3, 1, r), x[torch.as_tensor(shards[r])], beta.tolist(), gs[0], ds[r], dev)
             for r in range(3)]
    lc = LocalComm(steps)
    for r in range(6):
        lc.round(r, graph=True)
    ref = steps[0].losses_log(1, 6)
    for ln, rec in zip(lines, ref):
        got = json.loads(ln)
        assert got.pop("s") >= 0
        assert got == {"round": rec["round"], "server": 0, "d_loss": rec["d_loss"], "g_loss": rec["g_loss"],
                       "lambda": rec["lambda"], "F": rec["F"]}
    torch.cuda.synchronize()
    assert torch.equal(drv.step.g_params, steps[0].g_params)
    for w, s in enumerate(steps):
        assert torch.equal(drv.step.d_params[w], s.d_params), w
