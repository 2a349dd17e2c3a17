"""Interleaved A/B of the conv GAN round with fp32 and bf16 MFMA operands (ConvGanStep(gemm_dtype=)).

One process, one session: two steps at B = 256 over the same 60,000 resident rows (graph=True), each replaying
10-round graphs (run_rounds(10)); the legs alternate fp32 / bf16, 3 legs each, 200 rounds per leg after warm-up, and
the ms per round of every leg is printed.  ``--leg f32|bf16`` runs that step alone (for a kernel trace in a run of
its own: rocprofv3 --kernel-trace --stats -- python tools/conv_bf16_ab.py --leg bf16).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "cgl-gan_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rows", type=int, default=60000)
    ap.add_argument("--legs", type=int, default=3, help="legs per operand type")
    ap.add_argument("--rounds", type=int, default=200, help="timed rounds per leg")
    ap.add_argument("--chunk", type=int, default=10, help="rounds per graph replay (run_rounds)")
    ap.add_argument("--warmup", type=int, default=30, help="untimed rounds per step before the first leg")
    ap.add_argument("--leg", choices=["f32", "bf16"], default=None, help="time this operand type alone")
    a = ap.parse_args()
    from cglgan.conv_step import ConvGanStep
    kinds = [a.leg] if a.leg else ["f32", "bf16"]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        data = torch.rand(a.rows, 1024, device="cuda", generator=torch.Generator("cuda").manual_seed(1000)) * 2 - 1
        steps = {}
        for k in kinds:
            st = ConvGanStep(a.batch, data=data, seed=20211212, graph=True, gemm_dtype=k)
            st.init_default(20211212, 20211213)
            st.run()                        # round 0 eager
            st.prepare_rounds(a.chunk)
            for _ in range(max(a.warmup // a.chunk, 1)):
                st.run_rounds(a.chunk)
            steps[k] = st
        torch.cuda.synchronize()
        print(f"conv GAN round, B={a.batch}, {a.rows} resident rows, graph replay of {a.chunk}-round graphs, "
              f"{a.rounds} rounds per leg, {torch.cuda.get_device_name(0)}")
        ms = {k: [] for k in kinds}
        for leg in range(a.legs):
            for k in kinds:
                st = steps[k]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.rounds // a.chunk):
                    st.run_rounds(a.chunk)
                torch.cuda.synchronize()
                v = (time.perf_counter() - t0) / (a.rounds // a.chunk * a.chunk) * 1e3
                ms[k].append(v)
                print(f"leg {leg} {k:>4}: {v:.4f} ms/round")
        for k in kinds:
            s = steps[k].stats()
            print(f"{k:>4}: mean {sum(ms[k]) / len(ms[k]):.4f} ms/round, min {min(ms[k]):.4f}, max {max(ms[k]):.4f}; "
                  f"after round {s['round']}: d_loss {s['d_loss']:.6f} g_loss {s['g_loss']:.6f}")
        if len(kinds) == 2:
            f, b = sum(ms["f32"]) / len(ms["f32"]), sum(ms["bf16"]) / len(ms["bf16"])
            print(f"bf16 / f32 = {b / f:.4f} ({(1 - b / f) * 100:+.1f} % time saved)")


if __name__ == "__main__":
    main()
