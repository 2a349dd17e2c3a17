"""Interleaved A/B on one GPU: W workers of one server as

  A  the lockstep path: W GanStep contexts (n_workers = W, rank r) under cglgan.exchange.LocalComm, graph=True --
     every context runs its own G forward / backward / Adam and its own chain of D launches, the exchange is torch ops;
  B  one co-located step (GanStep(colocated=W)) with run_rounds(10): G once, every D stage one launch over the W
     workers, ten rounds per hipGraph launch.

Both on the same shards, seed and initial state (device sampler, z drawn on device).  Per shape: warm-up, then
``--reps`` alternating windows of ``--rounds`` rounds each, every window timed with a host clock around work that
ends in a device synchronise; reports each side's ms per round (median and range over the windows), launches per
round and plan_info GEMM FLOPs per round.  With ``--timeline`` the co-located round's per-launch device times
(profile_round) are printed too.

``--mixg``: the Mix-G group instead (mixed-gan.py:238-292) -- A = W ``mixgen_worker(h)`` contexts (exchange at the
head layer, weighting mix_single), each recomputing the shared trunk, graph per phase; B = the co-located step over
the server's whole ``MixGenerator`` (``specs.mixgen_group(W)``): the trunk once, the heads W-grouped.  "Same
trajectory" then compares the trunk and every head with its context's.

    python tools/colocated_ab.py [--shapes 10x100,8x256] [--rounds 100] [--reps 5] [--timeline]
    python tools/colocated_ab.py --mixg --shapes 2x100,4x100 --timeline
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cgl-gan_amd"))

import torch  # noqa: E402

from cglgan import GanStep, specs  # noqa: E402
from cglgan.exchange import LocalComm  # noqa: E402
from cglgan.init import mixgen_state, topology_state  # noqa: E402

K = 10      # rounds per graph launch of the co-located step


def build(W, B, rows=1000, seed=20211212):
    gm, dm = specs.mnist_generator(), specs.mnist_discriminator()
    gs, ds = topology_state("capgan", 1, W, seed, 784)
    real = (torch.rand(W * rows, 784, generator=torch.Generator().manual_seed(1)) * 2 - 1).cuda()
    kw = dict(batch=B, gen_z=True, seed=seed)
    steps = []
    for r in range(W):
        s = GanStep(gm, dm, n_workers=W, rank=r, real=real[r * rows:(r + 1) * rows], sample_n=rows, **kw)
        s.load_state_dicts(gs[0], ds[r])
        s.reset()
        steps.append(s)
    co = GanStep(gm, dm, colocated=W, real=real, sample_n=rows, **kw)
    co.load_state_dicts(gs[0], ds)
    co.reset()
    return steps, co


def build_mixg(W, B, rows=1000, seed=20211212):
    group, dm = specs.mixgen_group(W), specs.mnist_discriminator()
    g_sd, d_sds = mixgen_state(W, seed=seed, n_discriminators=W)
    real = (torch.rand(W * rows, 784, generator=torch.Generator().manual_seed(1)) * 2 - 1).cuda()
    kw = dict(batch=B, gen_z=True, seed=seed, weighting="mix_single", exchange_layer=group.head_layer)
    steps = []
    for h in range(W):
        s = GanStep(group.head_spec(h), dm, n_workers=W, rank=h, real=real[h * rows:(h + 1) * rows], sample_n=rows,
                    **kw)
        s.load_state_dicts(g_sd, d_sds[h])
        s.reset()
        steps.append(s)
    co = GanStep(group, dm, colocated=W, real=real, sample_n=rows, **kw)
    co.load_state_dicts(g_sd, d_sds)
    co.reset()
    return steps, co


def same_g(steps, co):
    """Bitwise the same generator on both sides: every tensor a context holds (the replicated G, or the trunk and
    its own head) against the co-located step's."""
    return all(torch.equal(co.g_views[k], v) for s in steps for k, v in s.g_views.items())


def window(fn, rounds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(rounds)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10x100,8x256", help="WxB list (workers x batch)")
    ap.add_argument("--rounds", type=int, default=100, help="rounds per timed window (a multiple of 10)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeline", action="store_true")
    ap.add_argument("--mixg", action="store_true", help="the Mix-G group (per-worker heads) instead of CAPGAN")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("colocated_ab needs the GPU")
    rounds = max(K, a.rounds // K * K)
    for shape in a.shapes.split(","):
        W, B = (int(v) for v in shape.split("x"))
        steps, co = (build_mixg if a.mixg else build)(W, B)
        lc = LocalComm(steps)
        done = [0]

        def run_a(n):
            for _ in range(n):
                lc.round(done[0], graph=True)
                done[0] += 1

        def run_b(n):
            for _ in range(n // K):
                co.run_rounds(K)

        co.prepare_rounds(K)
        run_a(2 * K)          # warm-up: graphs captured, code objects loaded
        run_b(2 * K)
        ta, tb = [], []
        for _ in range(a.reps):
            ta.append(window(run_a, rounds))
            tb.append(window(run_b, rounds))
        # same trajectory on both sides (same number of rounds run)
        same = same_g(steps, co)
        la = sum(len(s.launches()) for s in steps) + W      # + one alpha_scale launch per context (torch ops not counted)
        fa = sum(s.plan_info()["gemm_flops"] for s in steps)
        lb, fb = len(co.launches()), co.plan_info()["gemm_flops"]
        ma, mb = statistics.median(ta), statistics.median(tb)
        print(f"{'Mix-G ' if a.mixg else ''}W={W} B={B}  rounds/window={rounds} windows={a.reps} (alternating)  same_trajectory={same}")
        print(f"  A lockstep   : {ma:8.4f} ms/round (min {min(ta):.4f} max {max(ta):.4f})  "
              f"launches/round {la}  gemm GFLOP/round {fa / 1e9:.3f}")
        print(f"  B co-located : {mb:8.4f} ms/round (min {min(tb):.4f} max {max(tb):.4f})  "
              f"launches/round {lb}  gemm GFLOP/round {fb / 1e9:.3f}")
        print(f"  A / B = {ma / mb:.2f}x", flush=True)
        if a.timeline:
            us = co.profile_round()
            for (kind, fl, grid), t in zip(co.launches(), us):
                print(f"    {kind:14s} grid {grid:6d}  {t:8.2f} us  {fl / 1e6:10.1f} MFLOP")
            print(f"    sum of launches {sum(us):.1f} us", flush=True)
        del steps, co, lc


if __name__ == "__main__":
    main()
