"""Host side of the device round log: the C entry points that need no device (capacity, argument checks), the
ctypes mirror of cgl_gan_round_rec, the driver's chunk planner and its rounds_per_launch knob."""
import ctypes

import pytest

from cglgan import _lib as C
from cglgan.driver import DriverConfig, plan_chunks

E_ARG = -1
MAX_GRAPH_ROUNDS = 64       # CGL_MAX_GRAPH_ROUNDS (include/cglgan.h)


def test_capacity_holds_several_launches():
    assert C.lib.cgl_gan_round_log_capacity() >= 4 * MAX_GRAPH_ROUNDS


def test_read_rejects_null_context():
    buf = (C.GanRoundRec * 1)()
    assert C.lib.cgl_gan_read_round_log(None, 1, 1, buf, None) == E_ARG


def test_record_is_whole_cache_lines():
    assert ctypes.sizeof(C.GanRoundRec) % 64 == 0
    # the fields the header lists, in its order, 32-bit words throughout (no hidden padding)
    names = [f[0] for f in C.GanRoundRec._fields_]
    assert names[:11] == ["round", "d_loss", "d_real", "d_fake", "g_loss", "alpha", "F", "lambda_", "real_rows",
                          "loss_scale", "step_skipped"]
    assert C.GanRoundRec.round.offset == 0 and C.GanRoundRec.g_loss.offset == 4 * 25
    assert C.GanRoundRec.real_rows.offset == 4 * 29 and C.GanRoundRec.step_skipped.offset == 4 * 39


@pytest.mark.parametrize("args,want", [
    ((0, 23, 10, 0), [10, 10, 3]),
    ((0, 23, 10, 8), [8, 8, 7]),
    ((5, 10, 4, 6), [1, 4, 2, 3]),
    ((0, 5, 1, 0), [1, 1, 1, 1, 1]),
    ((3, 4, 1, 2), [1, 1, 1, 1]),
    ((0, 0, 10, 0), []),
    ((7, 0, 10, 4), []),
])
def test_plan_chunks(args, want):
    got = plan_chunks(*args)
    assert got == want
    assert sum(got) == args[1]


def test_plan_chunks_capped_at_log_capacity():
    # a chunk must still be whole in the ring when it is read back
    assert plan_chunks(0, 10, 64, 0, log_capacity=4) == [4, 4, 2]
    assert plan_chunks(0, 10, 3, 0, log_capacity=4) == [3, 3, 3, 1]


def test_rounds_per_launch_validated():
    assert DriverConfig(num_workers=1).rounds_per_launch == 10
    for ok in (1, 10, MAX_GRAPH_ROUNDS):
        DriverConfig(num_workers=1, rounds_per_launch=ok).validate()
    for bad in (0, MAX_GRAPH_ROUNDS + 1, -3):
        with pytest.raises(ValueError):
            DriverConfig(num_workers=1, rounds_per_launch=bad).validate()


def test_rounds_per_launch_is_not_a_resume_key():
    from cglgan.driver import Driver
    assert "rounds_per_launch" not in Driver.RESUME_KEYS


def test_cli_flag():
    from cglgan.driver import parse_args
    assert parse_args([]).rounds_per_launch == 10
    assert parse_args(["--rounds_per_launch", "32"]).rounds_per_launch == 32
