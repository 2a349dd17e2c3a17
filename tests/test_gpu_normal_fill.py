"""The N(0,1) stream of cgl_normal_fill / cgl_normal_fill_dev: tail coverage and a pin of the stream itself.

The stream (cgl_common.h: cgl_philox + cgl_normal_at) is Philox4x32-10 with counter (q_lo, q_hi, round,
stream_id) and key = the two halves of the seed; thread q turns the four output words into outputs
4q .. 4q+3 by Box-Muller.  Checkpoints and resume depend on it, so it is restated here on the host
(numpy), the restatement is checked against the Random123 known answers on the CPU, and the GPU fills
are compared with it value by value.

Tolerance of the GPU comparison: the host evaluates log / sqrt / sin / cos in fp64 from the same fp32
u1, u2 and the same fp32 sincos argument; the device's logf, sqrtf and sincosf are each within 2 ulp,
compounded and doubled: 16 ulp(max(|z|, 1)).  Worst ratio to that bound measured on the MI355X: 0.20.
"""
import ctypes

import numpy as np
import pytest
import torch

from philox_ref import KAT, M32, philox4x32_10

gpu = pytest.mark.gpu


def test_philox_known_answers():
    for ctr, key, out in KAT:
        got = philox4x32_10(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32))
        assert [int(v) for v in got] == out
    # vectorised form: the three vectors at once
    got = philox4x32_10(np.array([k[0] for k in KAT], dtype=np.uint32), np.array([k[1] for k in KAT], dtype=np.uint32))
    assert got.tolist() == [k[2] for k in KAT]


def normal_ref(n, seed, rnd, stream_id):
    """fp64 host value of outputs [0, n) of the stream (seed, round, stream_id): u1, u2 and the sincos
    argument formed in fp32 exactly as cgl_normal_at does, log / sqrt / sin / cos in fp64."""
    nq = (n + 3) // 4
    q = np.arange(nq, dtype=np.uint64)
    ctr = np.stack([q & M32, q >> np.uint64(32), np.full(nq, rnd & 0xFFFFFFFF, dtype=np.uint64),
                    np.full(nq, stream_id & 0xFFFFFFFF, dtype=np.uint64)], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    w = philox4x32_10(ctr, np.broadcast_to(key, (nq, 2)))
    inv = np.float32(2.3283064365386963e-10)
    z = np.empty((nq, 4), dtype=np.float64)
    for j in range(2):
        u1 = (w[:, 2 * j].astype(np.float32) + np.float32(1.0)) * inv
        u2 = w[:, 2 * j + 1].astype(np.float32) * inv
        arg = (np.float32(6.283185307179586) * u2).astype(np.float32)
        assert u1.dtype == np.float32 and arg.dtype == np.float32
        rr = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
        z[:, 2 * j] = rr * np.cos(arg.astype(np.float64))
        z[:, 2 * j + 1] = rr * np.sin(arg.astype(np.float64))
    return z.reshape(-1)[:n]


def test_host_reference_is_standard_normal():
    z = normal_ref(1 << 16, 1234, 0, 0)
    assert np.isfinite(z).all()
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02
    assert not np.array_equal(z, normal_ref(1 << 16, 1234, 1, 0))


# ---------------------------------------------------------------------------------------------------
def _lib():
    from cglgan import _lib as C
    return C


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


SENT = 8          # sentinel words past n
PAT = 0x7FC0BEEF  # the pre-fill: a NaN with a payload (a missed output stays NaN, a stray store changes the word)


def _fill(entry, n, seed, rnd, sid):
    """One fill of n values into a NaN-pattern buffer of n + SENT words; returns the whole buffer (int32 view
    on the CPU).  entry: 'host' cgl_normal_fill, 'dev' cgl_normal_fill_dev, 'batch' the latter inside a launch batch."""
    C = _lib()
    buf = torch.full((n + SENT,), PAT, dtype=torch.int32, device="cuda").view(torch.float32)
    useed = seed & (2 ** 64 - 1)
    if entry == "host":
        C.check(C.lib.cgl_normal_fill(_p(buf), n, useed, rnd, sid, _s()))
    else:
        rd = torch.tensor([rnd], dtype=torch.int32, device="cuda")
        if entry == "dev":
            C.check(C.lib.cgl_normal_fill_dev(_p(buf), n, useed, _p(rd), sid, _s()))
        else:
            from cglgan import conv_ops
            with conv_ops.launch_batch():
                C.check(C.lib.cgl_normal_fill_dev(_p(buf), n, useed, _p(rd), sid, _s()))
    torch.cuda.synchronize()
    return buf.view(torch.int32).cpu()


@gpu
@pytest.mark.parametrize("entry", ["host", "dev", "batch"])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 1025, 1027, 2049])
def test_tail_is_written(entry, n):
    """Every one of the n outputs is written, for n that is no multiple of 4 too (the launch covers
    ceil(n / 4) threads: with n / 4 threads, n = 1025 left out[1024] untouched and n < 4 launched nothing),
    nothing past n is, and the values are the first n of the 4 ceil(n / 4) fill."""
    seed, rnd, sid = 99, 3, 1
    got = _fill(entry, n, seed, rnd, sid)
    vals = got[:n].view(torch.float32)
    assert torch.isfinite(vals).all(), f"unwritten outputs at {torch.nonzero(~torch.isfinite(vals)).flatten().tolist()}"
    assert (got[n:] == PAT).all(), "sentinel words past n overwritten"
    n4 = 4 * ((n + 3) // 4)
    full = _fill(entry, n4, seed, rnd, sid)
    assert torch.equal(got[:n], full[:n])
    assert (full[n4:] == PAT).all()


@gpu
def test_n_zero_and_bad_args():
    C = _lib()
    buf = torch.full((SENT,), PAT, dtype=torch.int32, device="cuda")
    rd = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert C.lib.cgl_normal_fill(_p(buf), 0, 1, 0, 0, _s()) == 0
    assert C.lib.cgl_normal_fill_dev(_p(buf), 0, 1, _p(rd), 0, _s()) == 0
    assert C.lib.cgl_normal_fill(None, 4, 1, 0, 0, _s()) == -1
    assert C.lib.cgl_normal_fill(_p(buf), -1, 1, 0, 0, _s()) == -1
    assert C.lib.cgl_normal_fill_dev(_p(buf), 4, 1, None, 0, _s()) == -1
    torch.cuda.synchronize()
    assert (buf.cpu() == PAT).all()


def _ratio(got, ref):
    """max |got - ref| / (16 ulp_fp32(max(|ref|, 1)))"""
    ulp = np.spacing(np.maximum(np.abs(ref), 1.0).astype(np.float32)).astype(np.float64)
    return float(np.max(np.abs(got.astype(np.float64) - ref) / (16.0 * ulp)))


STREAMS = [(1234, 0, 0, 4096), ((1 << 63) + 5, 7, 3, 4096), (1234, 2, 0, (1 << 20) + 1027)]


@gpu
@pytest.mark.parametrize("seed,rnd,sid,n", STREAMS)
def test_stream_matches_host_reference(seed, rnd, sid, n):
    """The device stream is the host restatement's, value by value, within 16 ulp(max(|z|, 1)).

    Measured on the MI355X (worst |err| / bound): 0.12, 0.16 and 0.20 for the three streams."""
    ref = normal_ref(n, seed, rnd, sid)
    got = _fill("host", n, seed, rnd, sid)
    assert (got[n:] == PAT).all()
    g = got[:n].view(torch.float32).numpy()
    r = _ratio(g, ref)
    print(f"normal_fill seed={seed} round={rnd} stream={sid} n={n}: worst ratio to bound {r:.4f}")
    assert r <= 1.0
    # the device-round entry point draws the same stream, bit for bit
    dev = _fill("dev", n, seed, rnd, sid)
    assert torch.equal(dev, got)


@gpu
def test_round_and_stream_id_select_the_stream():
    n = 4096
    base = _fill("host", n, 1234, 0, 0)[:n]
    for rnd, sid in ((1, 0), (0, 1)):
        other = _fill("host", n, 1234, rnd, sid)[:n]
        assert not torch.equal(base, other)
        assert _ratio(other.view(torch.float32).numpy(), normal_ref(n, 1234, rnd, sid)) <= 1.0
    # the high half of the seed is key word 1
    hi = _fill("host", n, 1234 + (1 << 32), 0, 0)[:n]
    assert not torch.equal(base, hi)
    assert _ratio(hi.view(torch.float32).numpy(), normal_ref(n, 1234 + (1 << 32), 0, 0)) <= 1.0
