"""The conv round's device round log (cgl_conv_round_rec, ConvGanStep.losses_log): every way a round runs -- eager,
the one-round graph, K-round graphs, the split round's phase graphs, the separate launch of CGL_CONV_WDEFER=0 --
leaves the record the round's own ``stats()`` would have given, plus F, alpha, the real-row count and the Adam
steps; the ring wraps, a resume load clears it, and ``train_conv`` prints the per-round lines from it.

Every case runs at B = 8 on a shard of 3 B + 5 = 29 rows: a pass is batches of 8, 8, 8, 5, so a short batch and a
pass boundary fall inside a multi-round graph."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
B = 8
EPS = 2.0 ** -23
EXACT = ("round", "d_real", "d_fake", "d_loss", "g_loss", "lambda")


def _data(seed=7):
    return torch.rand(3 * B + 5, 1024, device="cuda", generator=torch.Generator("cuda").manual_seed(seed)) * 2 - 1


def _step(data, seed=23, graph=True, init=(8, 9), **kw):
    from cglgan.conv_step import ConvGanStep
    st = ConvGanStep(B, seed=seed, data=data, graph=graph, **kw)
    st.init_default(*init)
    return st


def _twin_rounds(b, n):
    """n rounds of ``b`` one at a time, each round's stats() + nv."""
    out = []
    for _ in range(n):
        b.run()
        st = b.stats()
        st["real_rows"] = int(b.nv.item())
        out.append(st)
    return out


def test_k_round_graphs_equal_round_by_round_twin():
    data = _data()
    a, b = _step(data), _step(data)
    a.run()
    for k in (3, 4, 2):
        a.run_rounds(k)
    want = _twin_rounds(b, 10)
    got = a.losses_log(1, 10)
    for g, w in zip(got, want):
        for k in EXACT:
            assert g[k] == w[k], (w["round"], k, g[k], w[k])
        assert g["real_rows"] == w["real_rows"]
        assert g["g_step"] == g["d_step"] == g["round"]
    assert [g["round"] for g in got] == list(range(1, 11))
    assert {g["real_rows"] for g in got} == {5, 8}
    last = a.stats()
    assert all(got[-1][k] == last[k] for k in EXACT)
    assert torch.equal(a.G.p, b.G.p) and torch.equal(a.D.p, b.D.p)
    assert a.losses_log(4, 5) == got[3:8]


def test_eager_rounds_with_explicit_real_batches():
    from cglgan.conv_step import ConvGanStep
    st = ConvGanStep(B, seed=3)
    st.init_default(1, 2)
    g = torch.Generator().manual_seed(4)
    rows = []
    for r, n in enumerate((8, 5, 8)):
        st.run(real=(torch.rand(n, 1, 32, 32, generator=g) * 2 - 1).cuda())
        rec, s = st.losses_log(r + 1, 1)[0], st.stats()
        assert all(rec[k] == s[k] for k in EXACT), (rec, s)
        assert rec["g_step"] == rec["d_step"] == r + 1
        rows.append(rec["real_rows"])
    assert rows == [8, 5, 8]


def test_F_and_alpha_one_worker():
    data = _data()
    a = _step(data)
    a.run()
    a.run_rounds(4)
    recs = a.losses_log(1, 5)
    lam_before = 0.0
    for r in recs:
        assert r["alpha"] == 1.0
        want = float(r["g_loss"]) - 0.001 * lam_before
        bound = 4 * EPS * (abs(float(r["g_loss"])) + 0.001 * abs(lam_before))
        print(f"round {r['round']}: F {r['F']!r} formula {want!r} |diff| {abs(r['F'] - want):.3e} bound {bound:.3e}")
        assert abs(float(r["F"]) - want) <= bound
        lam_before = float(r["lambda"])


def test_records_against_conv_oracle():
    """A 3-round eager trajectory driven as tests/test_gpu_conv_step.py drives its own: the logged losses within
    its tolerance (``_check``: STEP_TOL of fp64, or 4x the fp32 oracle's own error) of the oracle's."""
    from test_gpu_conv_step import _check, _run
    st, o64, o32, outs = _run(B, "mse", seed=5, rounds=3)
    recs = st.losses_log(1, 3)
    fails = []
    for rec, (s, r64, r32, _, _) in zip(recs, outs):
        for k in ("d_real", "d_fake", "g_loss"):
            print(f"round {rec['round']} {k}: log {rec[k]!r} fp64 {float(r64[k])!r} fp32 {float(r32[k])!r}")
            assert rec[k] == s[k]
            _check(f"round {rec['round']} {k}", torch.tensor(rec[k]), torch.tensor(r64[k]), torch.tensor(r32[k]), fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("weighting", ["capgan", "mean"])
def test_two_workers_local_comm(weighting):
    from cglgan import conv_ops as O
    from cglgan.conv_step import ConvGanStep
    from cglgan.exchange import ConvLocalComm
    N, rounds = 2, 4
    ss = []
    for r in range(N):
        g = torch.Generator().manual_seed(40 + r)
        data = (torch.rand(3 * B + 5, 1024, generator=g) * 2 - 1).cuda()
        s = ConvGanStep(B, loss="mse", seed=11, n_workers=N, rank=r, weighting=weighting, data=data, graph=True,
                        beta=[0.4, 0.6])
        s.init_default(20211212, 20211213 + r)
        ss.append(s)
    comm = ConvLocalComm(ss)
    for r in range(rounds):
        lam_before = [s.lam for s in ss]
        comm.round(r, eager=r % 2 == 0)
        recs = [s.losses_log(r + 1, 1)[0] for s in ss]
        for s, rec, lb in zip(ss, recs, lam_before):
            assert rec["round"] == r + 1 and rec["lambda"] == s.lam
            al = torch.zeros(N, device="cuda")
            O.weights_scale(weighting, lb, s.beta, s.losses_all, s.rank, None, alpha_out=al)
            assert rec["alpha"] == float(al[s.rank])
            assert rec["g_loss"] == float(s.losses_all[s.rank])
            l64, a64 = s.losses_all.double().cpu(), al.double().cpu()
            want = float((a64 * l64).sum()) - 0.001 * lb
            bound = 8 * EPS * (float((a64 * l64).abs().sum()) + 0.001 * abs(lb))
            print(f"{weighting} round {r + 1} rank {s.rank}: F {rec['F']!r} formula {want!r} bound {bound:.3e}")
            assert abs(float(rec["F"]) - want) <= bound
        assert recs[0]["F"] == recs[1]["F"] and recs[0]["lambda"] == recs[1]["lambda"]
        assert abs(recs[0]["alpha"] + recs[1]["alpha"] - 1.0) <= 1e-6
        if weighting == "capgan":
            assert recs[0]["alpha"] != recs[1]["alpha"]
        else:
            assert recs[0]["lambda"] == 0.0 and recs[0]["alpha"] == recs[1]["alpha"] == 0.5
    assert ss[0]._phase_graphs is not None, "phase graphs never captured"


def test_ring_wrap():
    data = _data()
    a = _step(data)
    cap = a.log_capacity
    total = 2 * cap + 7
    a.run()
    done = 1
    while done < total:
        k = min(32, total - done)
        a.run_rounds(k)
        done += k
    assert a.round == total
    recs = a.losses_log(total - cap + 1, cap)
    assert [r["round"] for r in recs] == list(range(total - cap + 1, total + 1))
    # rounds 2 cap - 2 .. 2 cap + 3 lie across the physical end of the ring (round 2 cap sits in the last slot)
    first = 2 * cap - 2
    assert a.losses_log(first, 6) == [a.losses_log(first + i, 1)[0] for i in range(6)]
    for first, count in ((1, 7), (total - cap - 2, 5), (total - 2, 5)):
        with pytest.raises(LookupError):
            a.losses_log(first, count)
    for first, count in ((total - cap + 1, cap + 1), (0, 3)):
        with pytest.raises((ValueError, LookupError)):
            a.losses_log(first, count)


def test_resume_clears_the_log():
    data = _data()
    twin, src, dst = _step(data), _step(data), _step(data, init=(3, 4))
    for _ in range(3):
        src.run()
    sd = src.resume_state()
    for _ in range(6):
        dst.run()
        twin.run()
    assert [r["round"] for r in dst.losses_log(1, 6)] == list(range(1, 7))
    dst.load_resume_state(sd)
    for first, count in ((1, 6), (1, 3), (3, 1), (4, 3), (6, 1)):
        with pytest.raises(LookupError):
            dst.losses_log(first, count)
    dst.run_rounds(3)
    assert dst.losses_log(4, 3) == twin.losses_log(4, 3)
    with pytest.raises(LookupError):
        dst.losses_log(3, 2)
    assert dst.round == twin.round == 6
    assert torch.equal(dst.G.p, twin.G.p) and torch.equal(dst.D.p, twin.D.p)


def test_fresh_step_has_an_empty_log():
    a = _step(_data())
    assert a.log_capacity >= 256
    for first, count in ((1, 1), (1, a.log_capacity), (5, 3)):
        with pytest.raises(LookupError):
            a.losses_log(first, count)


_CHILD = """
import json, sys, torch
sys.path[:0] = {paths!r}
from test_gpu_conv_round_log import _data, _step
a = _step(_data())
assert a.wdefer == (sys.argv[1] == "1")
a.run()
a.run_rounds(3)
print("RECS " + json.dumps([[r[k] for k in sorted(r)] for r in a.losses_log(1, 4)]))
"""


def test_separate_launch_without_the_deferred_one():
    """CGL_CONV_WDEFER=0 (read at construction, so in a child process): cgl_conv_round_log's own launch gives the
    records of the default build, whose deferred launch carries them."""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    code = _CHILD.format(paths=[root, os.path.join(root, "cgl-gan_amd"), here])
    env = dict(os.environ, CGL_CONV_WDEFER="0")
    out = subprocess.run([sys.executable, "-c", code, "0"], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RECS ")][-1][5:])
    a = _step(_data())
    assert a.wdefer
    a.run()
    a.run_rounds(3)
    want = [[r[k] for k in sorted(r)] for r in a.losses_log(1, 4)]
    assert got == want


def test_kgraph_cache_is_bounded():
    data = _data()
    a, b = _step(data), _step(data)
    a.run()
    b.run()
    for k in (2, 3, 4, 5, 6):
        a.run_rounds(k)
        assert len(a._kgraphs) <= 4
        for _ in range(k):
            b.run()
    assert list(a._kgraphs) == [3, 4, 5, 6]
    assert a.round == b.round == 21 and a.lam == b.lam
    assert torch.equal(a.G.p, b.G.p) and torch.equal(a.D.p, b.D.p)
    assert a.losses_log(1, 21) == b.losses_log(1, 21)


@pytest.mark.parametrize("log_every", [1, 3])
def test_train_conv_lines(log_every):
    from cglgan.conv_driver import train_conv
    data = _data()
    out = []
    for k in (4, 1):
        a = _step(data)
        a.run()
        lines = []
        lams = train_conv(a, 9, rounds_per_launch=k, log_every=log_every, log=lines.append)
        recs = [json.loads(ln) for ln in lines]
        assert [r["round"] for r in recs] == [r for r in range(2, 11) if r % log_every == 0]
        assert lams == [r["lambda"] for r in recs]
        assert set(recs[0]) == {"round", "server", "d_loss", "g_loss", "lambda", "F", "s"}
        for r in recs:
            r.pop("s")
        out.append(recs)
        assert a.round == 10
        assert recs[-1]["lambda"] == a.losses_log(recs[-1]["round"], 1)[0]["lambda"]
    assert out[0] == out[1]
