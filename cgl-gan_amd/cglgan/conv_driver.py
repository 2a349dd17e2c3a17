"""A runner for the conv GAN round (cglgan.conv_step.ConvGanStep) that issues multi-round graphs and still logs
every round: the reference's per-round line (F and Lambda, capgan.py:177-183) read from the device round log.

The conv model is not part of cglgan.driver.Driver (no conv topology initialisation or checkpoints yet); this is
the loop a caller writes around a ConvGanStep or a ConvWorkerExchange, with Driver.run's launch / read / emit order.
"""
from __future__ import annotations

import json
import time

from .driver import plan_chunks


def train_conv(target, rounds, rounds_per_launch=10, log_every=0, log=print, start_round=None):
    """``rounds`` rounds of ``target`` -- a ConvGanStep (N = 1, or co-located: its lines carry worker 0's losses and
    the server's F / lambda), a ConvWorkerExchange or a ConvColocatedExchange -- in launches of up to
    ``rounds_per_launch`` rounds (``run_rounds`` / ``exchange.rounds``: one hipGraph each on a one-worker graph
    step), cut by ``driver.plan_chunks`` and capped by the round log's capacity so that a whole launch is still in
    the ring when it is read.  With ``log_every`` a JSON line per due round with Driver.run's keys (``round,
    server, d_loss, g_loss, lambda, F, s``; ``s`` = host seconds since the call began when the line was emitted):
    after a launch the records of its due rounds are read with one copy, and their lines are formatted and emitted
    only after the NEXT launch has been issued, so the GPU works while the host formats.  ``start_round``: the
    rounds completed before the call (default: the step's own count).  Returns the lambdas of the logged rounds."""
    step = getattr(target, "step", target)
    if hasattr(target, "rounds"):
        issue = target.rounds
    else:
        issue = lambda r0, m: target.run_rounds(m)
    done = int(step.round if start_round is None else start_round)
    lambdas = []
    t0 = time.perf_counter()

    def emit(held):
        due, recs = held
        for r, st in zip(due, step.log_dicts(recs)[::log_every]):
            lambdas.append(st["lambda"])
            if log is not None:
                log(json.dumps({"round": r, "server": 0, "d_loss": st["d_loss"], "g_loss": st["g_loss"],
                                "lambda": st["lambda"], "F": st["F"], "s": round(time.perf_counter() - t0, 3)}))

    held = None     # (rounds due, their records) of the launch before the running one
    for m in plan_chunks(done, rounds, rounds_per_launch, 0, step.log_capacity):
        issue(done, m)
        if held is not None:
            emit(held)
            held = None
        first = done + 1
        done += m
        due = [r for r in range(first, done + 1) if log_every and r % log_every == 0]
        if due:
            held = (due, step.read_log(due[0], due[-1] - due[0] + 1))
    if held is not None:
        emit(held)
    return lambdas
