"""cglgan.driver on multi-round graph launches: Driver.run cuts the rounds into launches of rounds_per_launch rounds
(plan_chunks) and reads the per-round log lines from the device round log, so the drop-in driver runs the path
bench.py times.  The knob must not change anything a user can observe but the time stamps: same log lines, same
lambda_list, bitwise the same parameters as one graph launch per round."""
import functools
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROUNDS = 23


def _cfg(algo="capgan", **kw):
    from cglgan.driver import DriverConfig
    base = dict(algo=algo, num_workers=1, batch_size=64, num_communication=ROUNDS, dataset_rows=4000, num_sample=100,
                log_every=1)
    base.update(kw)
    return DriverConfig(**base)


def _run(cfg):
    """(log lines without the time stamp, lambda_list, g_params, d_params, run_rounds counts, stats() calls)."""
    from cglgan.driver import Driver
    drv = Driver(cfg)
    counts, stats_calls = [], []
    rr, st = drv.step.run_rounds, drv.step.stats

    def run_rounds(n, graph=True):
        counts.append(n)
        return rr(n, graph=graph)

    def stats():
        stats_calls.append(drv.round)
        return st()

    drv.step.run_rounds, drv.step.stats = run_rounds, stats
    lines = []
    final = drv.run(log=lines.append)
    torch.cuda.synchronize()
    parsed = [json.loads(ln) for ln in lines]
    assert all("s" in p for p in parsed)
    for p in parsed:
        del p["s"]
    return dict(lines=parsed, lambdas=list(drv.lambda_list), g=drv.step.g_params.clone(), d=drv.step.d_params.clone(),
                counts=counts, stats_calls=stats_calls, final=final)


@functools.lru_cache(maxsize=None)
def _reference(algo):
    """One graph launch per round with a line after every round: what every other setting must reproduce."""
    return _run(_cfg(algo, rounds_per_launch=1))


@pytest.mark.parametrize("algo", ["capgan", "mdgan"])
def test_same_trajectory_and_lines(algo):
    one, ten = _reference(algo), _run(_cfg(algo, rounds_per_launch=10))
    assert len(ten["lines"]) == ROUNDS and [p["round"] for p in ten["lines"]] == list(range(1, ROUNDS + 1))
    assert set(ten["lines"][0]) == {"round", "server", "d_loss", "g_loss", "lambda", "F"}
    assert ten["lines"] == one["lines"]
    assert ten["lambdas"] == one["lambdas"] and len(ten["lambdas"]) == ROUNDS
    assert torch.equal(ten["g"], one["g"]) and torch.equal(ten["d"], one["d"])
    assert ten["final"]["round"] == ROUNDS
    # the last line is the round the final stats() describes
    assert ten["lines"][-1]["g_loss"] == ten["final"]["g_loss"] and ten["lines"][-1]["F"] == ten["final"]["F"]


def test_chunks_issued():
    ten = _run(_cfg(rounds_per_launch=10))
    assert ten["counts"] == [10, 10, 3]
    assert ten["stats_calls"] == [ROUNDS]            # only the stats() Driver.run returns, after the last round
    assert _reference("capgan")["counts"] == [1] * ROUNDS
    assert _reference("capgan")["stats_calls"] == [ROUNDS]


def test_chunks_end_at_resume_points(tmp_path):
    from cglgan.driver import Driver
    cfg = _cfg(rounds_per_launch=10, resume_every=8, resume_dir=str(tmp_path))
    seen = []
    import cglgan.checkpoint as ck
    save = ck.save_resume

    def spy(step, path, **kw):
        seen.append((kw["round"], len(kw["lambda_list"])))
        return save(step, path, **kw)

    ck.save_resume = spy
    try:
        r = _run(cfg)
    finally:
        ck.save_resume = save
    assert r["counts"] == [8, 8, 7]
    assert os.path.exists(os.path.join(str(tmp_path), "resume-capgan-rank0.pt"))
    # written at rounds 8 and 16 and at the end, each holding the lambdas of the rounds logged before it (the
    # place the file has in the sequence of a round-by-round run: before its own round's line)
    assert seen == [(8, 7), (16, 15), (ROUNDS, ROUNDS)]
    assert r["lines"] == _reference("capgan")["lines"]
    assert torch.equal(r["g"], _reference("capgan")["g"])
    # and the file resumes: a new driver on the same directory has nothing left to run
    again = Driver(cfg)
    assert again.round == ROUNDS and again.lambda_list == r["lambdas"]


def test_log_every_5():
    five = _run(_cfg(rounds_per_launch=10, log_every=5))
    assert five["counts"] == [10, 10, 3]
    assert [p["round"] for p in five["lines"]] == [5, 10, 15, 20]
    ref = {p["round"]: p for p in _reference("capgan")["lines"]}
    assert five["lines"] == [ref[r] for r in (5, 10, 15, 20)]
    assert five["lambdas"] == [ref[r]["lambda"] for r in (5, 10, 15, 20)]
    assert torch.equal(five["g"], _reference("capgan")["g"])


def test_one_read_per_launch():
    from cglgan.driver import Driver
    drv = Driver(_cfg(rounds_per_launch=10))
    reads = []
    rl = drv.step.read_log
    drv.step.read_log = lambda *a: reads.append(a) or rl(*a)
    drv.run(log=None)
    assert reads == [(1, 10), (11, 10), (21, 3)]
    assert drv.lambda_list == _reference("capgan")["lambdas"]


def test_no_log_no_read():
    """log_every = 0: nothing is read between the launches."""
    from cglgan.driver import Driver
    drv = Driver(_cfg(log_every=0))
    reads = []
    ll, rl = drv.step.losses_log, drv.step.read_log
    drv.step.losses_log = lambda *a: reads.append(a) or ll(*a)
    drv.step.read_log = lambda *a: reads.append(a) or rl(*a)
    drv.run(log=None)
    assert reads == [] and drv.lambda_list == []
    assert torch.equal(drv.step.g_params, _reference("capgan")["g"])
