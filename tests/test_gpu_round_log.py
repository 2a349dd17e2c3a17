"""The device round log (cgl_gan_read_round_log / GanStep.losses_log): the scalar tail of every round's last launch
leaves the round's record in a ring in the context workspace, so the rounds inside a multi-round graph launch are
readable one by one -- what the reference prints after every communication round (capgan.py:177-183).

The log is a copy of values the round already computes, so every comparison with ``stats()`` taken round by round
on a twin step is exact (==), and the comparison with the CPU oracle uses the trajectory tolerance of
tests/test_gpu_step.py unchanged."""
import functools

import pytest
import torch

from parity_helpers import TRAJ_TOL, feed, inputs, make_pair, oracle_round, rel_scalar
from test_gpu_graph_rounds import _step

pytestmark = pytest.mark.gpu

STAT_KEYS = ("round", "d_loss", "d_real", "d_fake", "g_loss", "alpha", "F", "lambda")


@pytest.fixture(autouse=True)
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _assert_rec(rec, st, keys=STAT_KEYS, where=None):
    for k in keys:
        assert rec[k] == st[k], (where, k, rec[k], st[k])


def _single_rounds(step, n, graph=True):
    """n rounds one by one with a stats() (and the sampler's row counts) after each: the per-round truth."""
    out = []
    for _ in range(n):
        step.run(graph=graph)
        st = step.stats()
        st["real_rows"] = step.internal(4).view(torch.int32).cpu().tolist()
        out.append(st)
    return out


# ---------------------------------------------------------------- 1. K-round graphs vs single rounds
def test_graph_rounds_log_equals_single_round_stats():
    """150 resident rows at B = 64: two full batches and one of 22 per pass, so the short batch and the pass
    boundary fall inside a multi-round graph."""
    a, b = _step(B=64, rows=150), _step(B=64, rows=150)
    for n in (2, 5, 3, 7):
        a.run_rounds(n)
    want = _single_rounds(b, 17)
    got = a.losses_log(1, 17)
    assert len(got) == 17
    for r, (rec, st) in enumerate(zip(got, want), 1):
        assert rec["round"] == r
        _assert_rec(rec, st, where=r)
        assert rec["real_rows"] == st["real_rows"], (r, rec["real_rows"], st["real_rows"])
    assert sorted({rec["real_rows"][0] for rec in got}) == [22, 64]      # the short batch was inside the graphs
    _assert_rec(got[-1], a.stats(), where="last record vs stats()")
    assert torch.equal(a.g_params, b.g_params)
    # any sub-range reads the same records
    assert a.losses_log(6, 4) == got[5:9]


# ---------------------------------------------------------------- 2. eager rounds, two local D steps
def test_eager_epoch2_log():
    _, _, step = make_pair("capgan", 64, 40, 2)
    want = []
    for t in range(3):
        z1, z2, reals = inputs("capgan", 64, 40, 2, seed=700 + t)
        feed(step, z1, z2, reals)
        step.run(graph=False)
        want.append(step.stats())
    got = step.losses_log(1, 3)
    for r, (rec, st) in enumerate(zip(got, want), 1):
        _assert_rec(rec, st, where=r)
        assert len(rec["d_loss"]) == len(rec["d_real"]) == len(rec["d_fake"]) == 2
        assert all(v > 0.0 for v in rec["d_loss"]), rec       # both local D steps left their loss
    assert got[0]["d_loss"][0] != got[0]["d_loss"][1]


# ---------------------------------------------------------------- 3. against the CPU oracle
@pytest.mark.parametrize("kind", ["capgan", "mdgan", "ring"])
def test_log_against_oracle(kind):
    srv, workers, step = make_pair(kind, 64)
    fed = []
    for t in range(10):
        z1, z2, reals = inputs(kind, 64, 64, 1, seed=100 + t)
        feed(step, z1, z2, reals)
        step.run(graph=(t % 2 == 1))
        fed.append((z1, z2, reals))
    got = step.losses_log(1, 10)        # the only host read of the ten rounds
    for t, (rec, (z1, z2, reals)) in enumerate(zip(got, fed)):
        r = oracle_round(kind, srv, workers, z1, z2, reals)
        assert rec["round"] == t + 1
        assert rel_scalar(rec["d_loss"][0], r["d_losses"][0]) <= TRAJ_TOL, (t, rec, r["d_losses"])
        assert rel_scalar(rec["g_loss"], r["g_losses"][0]) <= TRAJ_TOL, (t, rec, r["g_losses"])
        assert abs(rec["lambda"] - float(r["lam"])) <= 1e-6 + TRAJ_TOL * abs(float(r["lam"]))


# ---------------------------------------------------------------- 4. N > 1
def _workers2():
    from cglgan import GanStep, specs
    from cglgan.init import default_init
    g = torch.Generator(device="cuda").manual_seed(1000)
    data = torch.rand(2, 150, 784, device="cuda", generator=g) * 2 - 1
    gm, dm = specs.mnist_generator(), specs.mnist_discriminator()
    steps = []
    for r in range(2):
        s = GanStep(gm, dm, batch=64, loss="ce", weighting="capgan", n_workers=2, rank=r, seed=20211212, gen_z=True,
                    real=data[r], sample_n=150)
        torch.manual_seed(20211212)
        default_init(gm, s.g_views)           # the replicated G
        torch.manual_seed(20211213 + r)
        default_init(dm, s.d_views)           # each worker's own D
        s.reset(beta=[0.4, 0.6])
        steps.append(s)
    return steps


def test_two_workers_log():
    from cglgan.exchange import LocalComm
    a, b = _workers2(), _workers2()
    ca, cb = LocalComm(a), LocalComm(b)
    want = [[], []]
    for r in range(4):
        ca.round(r, graph=(r % 2 == 1))       # split phase A / phase B, eager and through the phase graphs
        cb.round(r, graph=(r % 2 == 1))
        for w in range(2):
            want[w].append(b[w].stats())
    for w in range(2):
        got = a[w].losses_log(1, 4)
        for r, (rec, st) in enumerate(zip(got, want[w]), 1):
            _assert_rec(rec, st, keys=("round", "alpha", "F", "lambda", "g_loss", "d_loss"), where=(w, r))
    # the two workers weigh their losses differently (alpha from the gathered losses, beta 0.4 / 0.6) but share F
    l0, l1 = a[0].losses_log(1, 4), a[1].losses_log(1, 4)
    assert all(x["F"] == y["F"] and x["lambda"] == y["lambda"] for x, y in zip(l0, l1))
    assert all(x["alpha"] != y["alpha"] and abs(x["alpha"] + y["alpha"] - 1.0) < 1e-6 for x, y in zip(l0, l1))


# ---------------------------------------------------------------- 5. ring wrap and overwrite
@functools.lru_cache(maxsize=None)
def _ring_run():
    """The ring model run 2 * cap + 7 rounds on the device sampler (one run, shared; nothing below changes it)."""
    g = torch.Generator(device="cuda").manual_seed(5)
    data = torch.randn(300, 2, device="cuda", generator=g) * 0.7
    st = make_pair("ring", 64, gen_z=True, real=data, sample_n=300)[2]
    cap = st.log_capacity
    total = 2 * cap + 7
    done = 0
    while done < total:
        n = min(64, total - done)
        st.run_rounds(n)
        done += n
    return st, cap, total


def test_ring_last_capacity_rounds_readable():
    st, cap, total = _ring_run()
    assert st.stats()["round"] == total
    got = st.losses_log(total - cap + 1, cap)
    assert [r["round"] for r in got] == list(range(total - cap + 1, total + 1))
    assert got[-1]["F"] == st.stats()["F"] and got[-1]["g_loss"] == st.stats()["g_loss"]
    assert len({r["g_loss"] for r in got}) > cap // 2    # the records are the rounds' own, not one repeated


def test_ring_overwritten_rounds_raise():
    st, cap, total = _ring_run()
    with pytest.raises(LookupError, match=str(cap)):
        st.losses_log(1, 7)
    with pytest.raises(LookupError):
        st.losses_log(total - cap, 2)          # the first of the two was overwritten by the last round
    with pytest.raises(LookupError):
        st.losses_log(total, 2)                # the second has not run yet
    with pytest.raises((LookupError, ValueError, RuntimeError)):
        st.losses_log(total - cap + 1, cap + 1)
    with pytest.raises((LookupError, ValueError, RuntimeError)):
        st.losses_log(0, 1)


def test_ring_range_across_the_physical_end():
    st, cap, total = _ring_run()
    first = 2 * cap - 2                        # slots cap - 3, cap - 2, cap - 1, 0, 1, 2
    got = st.losses_log(first, 6)
    one = [st.losses_log(first + i, 1)[0] for i in range(6)]
    assert got == one
    assert [r["round"] for r in got] == list(range(first, first + 6))


# ---------------------------------------------------------------- 6. reset and resume
def _resume_step(seed_init):
    from test_gpu_resume import _mlp
    return _mlp(seed_init)


def test_reset_clears_log():
    st = _step(B=64, rows=150)
    st.run_rounds(3)
    assert [r["round"] for r in st.losses_log(1, 3)] == [1, 2, 3]
    st.reset()
    with pytest.raises(LookupError):
        st.losses_log(1, 1)
    st.run(graph=True)
    assert st.losses_log(1, 1)[0]["round"] == 1
    with pytest.raises(LookupError):
        st.losses_log(2, 1)                     # round 2 of the old timeline is gone


def test_fresh_step_has_empty_log():
    st = _step(B=64, rows=150)
    with pytest.raises(LookupError):
        st.losses_log(1, 1)


def test_resume_clears_and_continues_log():
    a, b, c = _resume_step(1), _resume_step(1), _resume_step(2)
    a.run_rounds(6)
    want = a.losses_log(1, 6)
    b.run_rounds(3)
    sd = b.resume_state()
    words = sd["device_state"].numel()
    c.run_rounds(6)                            # its own timeline: rounds 1 .. 6 of other weights in the log
    c.load_resume_state(sd)
    for first, count in ((4, 3), (1, 3), (6, 1)):
        with pytest.raises(LookupError):
            c.losses_log(first, count)
    c.run_rounds(3)
    assert c.losses_log(4, 3) == want[3:]
    assert torch.equal(a.g_params, c.g_params) and torch.equal(a.d_params, c.d_params)
    with pytest.raises(LookupError):
        c.losses_log(3, 1)                      # round 3 ran on another step
    # the saved device state is the round-state block alone, the size a file written before the log existed holds
    # (sizeof(CglStepState) / 4 = 270 words, read from that build: load_resume_state refuses any other size)
    assert words == 270 and c.resume_state()["device_state"].numel() == words


# ---------------------------------------------------------------- 7. loss scaling
@pytest.mark.parametrize("scale", [65536.0, 2.0 ** 40])
def test_loss_scale_fields(scale):
    """65536 is the issue's case; 2^40 overflows the fp16 gradients, so the records must show the skipped
    steps and the halving scale round by round."""
    def build():
        g = torch.Generator(device="cuda").manual_seed(1000)
        data = torch.rand(150, 784, device="cuda", generator=g) * 2 - 1
        return make_pair("capgan", 64, gen_z=True, gemm_dtype="f16", loss_scale=scale, real=data, sample_n=150)[2]
    a, b = build(), build()
    a.run_rounds(4)
    got = a.losses_log(1, 4)
    for r, rec in enumerate(got, 1):
        b.run(graph=True)
        st = b.stats()
        assert rec["loss_scale"] == st["loss_scale"], (r, rec, st)
        assert rec["step_skipped"] == st["last_skipped"], (r, rec, st)
        _assert_rec(rec, st, where=r)
    if scale > 65536.0:
        assert got[0]["step_skipped"] == [1, 1] and got[1]["loss_scale"] == [scale / 2, scale / 2], got


def test_fp32_records_carry_no_scaling():
    st = _step(B=64, rows=150)
    st.run_rounds(2)
    for rec in st.losses_log(1, 2):
        assert rec["loss_scale"] == st.stats()["loss_scale"] and rec["step_skipped"] == [0, 0]


# ---------------------------------------------------------------- 8. the round's launches are unchanged
# Recorded from the parent commit (the build without the round log) on an MI355X: plan_info()["launches"] and
# [(kind, grid)] of launches() for make_pair(kind, 64).  The log adds no launch and no workgroup.
_MNIST_HEAD = [("gemm_prologue", 17), ("gemm", 32), ("bn_apply", 304), ("gemm", 64), ("bn_apply", 544), ("gemm", 128),
               ("bn_apply", 864), ("gemm", 100), ("gemm", 64), ("gemm", 32), ("head", 816), ("gemm", 210),
               ("gemm", 400)]
_MNIST_TAIL = [("gemm", 32), ("gemm", 16), ("head", 528), ("gemm", 33), ("gemm", 50), ("gemm", 493), ("bn_bwd", 128),
               ("gemm", 576), ("bn_bwd", 64), ("gemm", 160), ("bn_bwd", 32), ("gemm", 48), ("gemm", 16),
               ("adam", 1475)]
PARENT_PLANS = {
    "capgan": (28, _MNIST_HEAD + [("adam", 278)] + _MNIST_TAIL),      # (D's Adam: two logits)
    "mdgan": (28, _MNIST_HEAD + [("adam", 277)] + _MNIST_TAIL),       # (one Sigmoid unit)
    "ring": (16, [("gemm_prologue", 5), ("gemm", 2), ("gemm", 4), ("gemm", 32), ("head", 33), ("gemm", 66),
                  ("gemm", 4), ("adam", 33), ("gemm", 2), ("gemm", 16), ("head", 16), ("gemm", 9), ("gemm", 2),
                  ("gemm", 3), ("gemm", 4), ("adam", 4)]),
}


@pytest.mark.parametrize("kind", ["capgan", "mdgan", "ring"])
def test_launch_plan_unchanged(kind):
    _, _, step = make_pair(kind, 64)
    n, kinds = PARENT_PLANS[kind]
    assert step.plan_info()["launches"] == n
    assert [(k, g) for k, _, g in step.launches()] == kinds
    assert sorted(step.LAUNCH_KINDS.items()) == [
        (0, "gemm"), (1, "head"), (2, "bn_bwd"), (3, "adam"), (4, "prologue"), (5, "bn_apply"), (6, "gemm_adam"),
        (7, "gemm_prologue"), (8, "alpha_combine")]
