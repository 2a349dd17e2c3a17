"""Interleaved A/B on one GPU: the W conv-GAN workers (model/lsgan.py) of one server as

  A  the lockstep path: W ConvGanStep contexts (n_workers = W, rank q, graph=True) under
     cglgan.exchange.ConvLocalComm -- every context runs its own G forward / backward / Adam and weight pack, phase A
     and phase B replay as two hipGraphs per context, the exchange between them is torch ops and W cgl_weights_scale
     launches;
  B  one co-located step (ConvGanStep(colocated=W, graph=True)) with run_rounds(10): G once, the W D stages one after
     the other, the exchange one launch, ten rounds per hipGraph launch.

Both on the same shards, seed and initial state, and after the same number of rounds both must hold bitwise the same
G (asserted).  Per shape: warm-up, then ``--reps`` alternating windows of ``--rounds`` rounds each, every window timed
with a host clock around work that ends in a device synchronise; reports each side's ms per round (median and range
over the windows).  Then the co-located round's split into its G part, its W x D part and the exchange, from events
around one eager round (ConvGanStep.profile_round: launch-bound parts read longer there than inside the graph).

    python tools/conv_colocated_ab.py [--shapes 10x64,4x256] [--rounds 50] [--reps 5]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cgl-gan_amd"))

import torch  # noqa: E402

from cglgan.conv_step import ConvGanStep  # noqa: E402
from cglgan.exchange import ConvLocalComm  # noqa: E402

K = 10      # rounds per graph launch of the co-located step


def build(W, B, rows=1000, seed=20211212):
    g = torch.Generator().manual_seed(1)
    shards = [(torch.rand(rows, 1024, generator=g) * 2 - 1).cuda() for _ in range(W)]
    steps = []
    for r in range(W):
        s = ConvGanStep(B, seed=seed, n_workers=W, rank=r, data=shards[r], graph=True)
        s.init_default(seed, seed + 1 + r)
        steps.append(s)
    co = ConvGanStep(B, seed=seed, colocated=W, data=shards, graph=True)
    co.init_default(seed, [seed + 1 + r for r in range(W)])
    return steps, co


def window(fn, rounds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(rounds)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10x64,4x256", help="WxB list (workers x batch)")
    ap.add_argument("--rounds", type=int, default=50, help="rounds per timed window (a multiple of 10)")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv_colocated_ab needs the GPU")
    rounds = max(K, a.rounds // K * K)
    for shape in a.shapes.split(","):
        W, B = (int(v) for v in shape.split("x"))
        steps, co = build(W, B)
        lc = ConvLocalComm(steps)
        done = [0]

        def run_a(n):
            for _ in range(n):
                lc.round(done[0])
                done[0] += 1

        def run_b(n):
            for _ in range(n // K):
                co.run_rounds(K)

        run_a(K)              # warm-up: graphs captured, code objects loaded (B: round 1 eager, then the replays)
        run_b(K)
        co.prepare_rounds(K)
        run_a(K)
        run_b(K)
        ta, tb = [], []
        for _ in range(a.reps):
            ta.append(window(run_a, rounds))
            tb.append(window(run_b, rounds))
        torch.cuda.synchronize()
        same = all(torch.equal(co.G.p, s.G.p) for s in steps) and all(
            torch.equal(co.Ds[q].p, s.D.p) for q, s in enumerate(steps))
        assert same and co.round == steps[0].round, "the two sides left the same trajectory"
        ma, mb = statistics.median(ta), statistics.median(tb)
        print(f"conv W={W} B={B}  rounds/window={rounds} windows={a.reps} (alternating)  same_G_and_D={same}")
        print(f"  A lockstep   : {ma:8.4f} ms/round (min {min(ta):.4f} max {max(ta):.4f})")
        print(f"  B co-located : {mb:8.4f} ms/round (min {min(tb):.4f} max {max(tb):.4f})")
        print(f"  A / B = {ma / mb:.2f}x   B's range {'below' if max(tb) < min(ta) else 'NOT below'} A's", flush=True)
        parts = [co.profile_round() for _ in range(3)][-1]
        tot = sum(parts.values())
        print("  co-located round, one eager round by events (us): " +
              "  ".join(f"{k} {v:.0f} ({100 * v / tot:.0f}%)" for k, v in parts.items()) + f"  sum {tot:.0f}",
              flush=True)
        del steps, co, lc


if __name__ == "__main__":
    main()
