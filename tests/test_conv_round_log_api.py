"""Host side of the conv round log: the C entry points that need no device (capacity, argument and call-order
checks), the ctypes mirror of cgl_conv_round_rec, and train_conv's chunking and emit order on a stub step."""
import ctypes
import json

from cglgan import _lib as C
from cglgan.conv_driver import train_conv
from cglgan.driver import MAX_ROUNDS_PER_LAUNCH

E_ARG, E_STATE = -1, -2


def test_capacity_holds_several_launches():
    assert C.lib.cgl_conv_round_log_capacity() == 256
    assert C.lib.cgl_conv_round_log_capacity() >= 4 * MAX_ROUNDS_PER_LAUNCH


def test_record_is_one_cache_line():
    assert ctypes.sizeof(C.ConvRoundRec) == 64
    names = [f[0] for f in C.ConvRoundRec._fields_]
    # the fields the header lists, in its order, 32-bit words throughout (no hidden padding)
    want = ["round", "d_real", "d_fake", "d_loss", "g_loss", "alpha", "F", "lambda_", "real_rows", "g_step", "d_step"]
    assert names[:11] == want
    for i, k in enumerate(want):
        assert getattr(C.ConvRoundRec, k).offset == 4 * i, k
    assert C.ConvRoundRec.reserved_.offset == 44


def test_read_rejects_bad_arguments_without_a_device():
    buf = (C.ConvRoundRec * 4)()
    ring = ctypes.c_void_p(4096)      # never dereferenced: every case below is refused before any copy
    read = C.lib.cgl_conv_read_round_log
    assert read(None, 1, 1, buf, None) == E_ARG
    assert read(ring, 1, 1, None, None) == E_ARG
    assert read(ring, 0, 1, buf, None) == E_ARG
    assert read(ring, -5, 1, buf, None) == E_ARG
    assert read(ring, 1, 0, buf, None) == E_ARG
    assert read(ring, 1, 257, buf, None) == E_ARG


def _args():
    a = C.ConvRoundLogArgs()
    a.ring, a.lam_dev, a.lbuf, a.nv = 4096, 8192, 12288, 16384     # recorded, never dereferenced on the host
    a.n_workers, a.rank, a.weighting, a.half = 1, 0, 0, 0.5
    a.round, a.g_step, a.d_step = 1, 1, 1
    return a


def test_defer_log_call_order():
    log = C.lib.cgl_conv_wgrad_defer_log
    a = _args()
    assert log(ctypes.byref(a)) == E_STATE                  # outside a deferral
    assert C.lib.cgl_conv_wgrad_defer_begin() == 0
    try:
        bad = _args()
        bad.ring = None
        assert log(ctypes.byref(bad)) == E_ARG
        bad = _args()
        bad.n_workers, bad.rank = 2, 1                      # two workers need losses_all and alpha_all
        assert log(ctypes.byref(bad)) == E_ARG
        bad = _args()
        bad.round = 0                                       # host integers count the completed round: >= 1
        assert log(ctypes.byref(bad)) == E_ARG
        assert log(None) == E_ARG
        assert log(ctypes.byref(a)) == 0
        assert log(ctypes.byref(a)) == E_STATE              # at most once per deferral
    finally:
        # the addresses above are fakes: drop the recorded block instead of launching it
        assert C.lib.cgl_conv_wgrad_defer_cancel() == 0
    assert C.lib.cgl_conv_wgrad_defer_cancel() == E_STATE
    assert C.lib.cgl_conv_wgrad_defer_end(None) == E_STATE


class _StubStep:
    """What train_conv needs of a step: run_rounds, read_log, log_dicts, log_capacity, round."""

    def __init__(self, cap=6):
        self.round, self.log_capacity, self.events = 0, cap, []

    def run_rounds(self, m):
        self.events.append(("launch", self.round + 1, m))
        self.round += m

    def read_log(self, first, count):
        assert first >= 1 and first + count - 1 <= self.round and count <= self.log_capacity
        self.events.append(("read", first, count))
        return list(range(first, first + count))

    def log_dicts(self, recs):
        return [{"round": r, "d_loss": 0.5 * r, "g_loss": 0.25 * r, "lambda": 1e-4 * r, "F": -1.0 * r} for r in recs]


def test_train_conv_chunks_and_emits_after_the_next_launch():
    st = _StubStep()
    st.round = 1
    lines = []

    def log(ln):
        st.events.append(("emit", json.loads(ln)["round"]))
        lines.append(json.loads(ln))

    lams = train_conv(st, 9, rounds_per_launch=4, log_every=2, log=log)
    assert st.round == 10
    assert st.events == [
        ("launch", 2, 4), ("read", 2, 3),                       # rounds 2 .. 5: due 2, 4
        ("launch", 6, 4), ("emit", 2), ("emit", 4), ("read", 6, 3),
        ("launch", 10, 1), ("emit", 6), ("emit", 8), ("read", 10, 1),
        ("emit", 10)]
    assert lams == [1e-4 * r for r in (2, 4, 6, 8, 10)]
    assert set(lines[0]) == {"round", "server", "d_loss", "g_loss", "lambda", "F", "s"}
    assert [ln["F"] for ln in lines] == [-2.0, -4.0, -6.0, -8.0, -10.0]


def test_train_conv_caps_a_launch_at_the_log_capacity():
    st = _StubStep(cap=6)
    assert train_conv(st, 14, rounds_per_launch=10, log_every=1, log=None, start_round=0) == \
        [1e-4 * r for r in range(1, 15)]
    assert [e for e in st.events if e[0] == "launch"] == [("launch", 1, 6), ("launch", 7, 6), ("launch", 13, 2)]


def test_train_conv_without_logging_reads_nothing():
    st = _StubStep()
    assert train_conv(st, 5, rounds_per_launch=2, log_every=0) == []
    assert st.events == [("launch", 1, 2), ("launch", 3, 2), ("launch", 5, 1)]
