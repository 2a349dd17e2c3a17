"""Argument checks of the co-located conv entry points, on the CPU: the exchange launch (cgl_conv_alpha_combine), the
grouped sampler and Dropout2d masks (cgl_sample_rows_dev_multi, cgl_dropout2d_masks_dev_multi and their _prepare
calls), cgl_bcast_rows and the grouped round log.  Every call here is refused on the host, or only recorded into an
open launch batch / weight-gradient deferral that is then cancelled: nothing reaches a launch, so the dummy address
4096 is never dereferenced (the style of test_conv_arg_checks.py)."""
import ctypes

import pytest

from cglgan import _lib as C

L = C.lib
E_ARG, E_STATE = -1, -2
P = ctypes.c_void_p(4096)
P4 = ctypes.c_void_p(4096 + 4)
NUL = ctypes.c_void_p(0)
S = ctypes.c_void_p(0)
BETA = (ctypes.c_float * 16)(*([1.0 / 16] * 16))

COMBINE_OK = dict(weighting=0, W=3, beta=BETA, gloss=P, gstride=8, lam=P, d=P, nx=1024, dimg=P, alpha=P, losses=P)


def _combine(**over):
    a = dict(COMBINE_OK, **over)
    return L.cgl_conv_alpha_combine(a["weighting"], a["W"], a["beta"], a["gloss"], a["gstride"], a["lam"], a["d"],
                                    a["nx"], a["dimg"], a["alpha"], a["losses"], S)


@pytest.mark.parametrize("over", [dict(gloss=NUL), dict(lam=NUL), dict(d=NUL), dict(dimg=NUL), dict(alpha=NUL),
                                  dict(losses=NUL), dict(beta=None), dict(d=P4), dict(dimg=P4), dict(W=1), dict(W=0),
                                  dict(W=17), dict(weighting=-1), dict(weighting=5), dict(nx=0), dict(nx=-4),
                                  dict(nx=1022), dict(nx=2), dict(gstride=0)])
def test_alpha_combine_refusals(over):
    assert _combine(**over) == E_ARG


def test_alpha_combine_not_batchable():
    """The exchange depends on the round's G-loss passes: it is not a round-start op, an open batch refuses it."""
    assert L.cgl_conv_batch_begin(S) == 0
    try:
        assert _combine() == E_STATE
    finally:
        assert L.cgl_conv_batch_cancel() == 0
    assert L.cgl_conv_batch_cancel() == E_STATE


def _sample(desc=P, blocks=24, rnd=P):
    return L.cgl_sample_rows_dev_multi(desc, blocks, rnd, S)


def _job(src=4096, dst=4096, nv=4096, n_src=20):
    j = C.SampleJob()
    j.src, j.dst, j.nv_out, j.seed, j.n_src = src, dst, nv, 5, n_src
    return j


def _sample_prepare(jobs, njobs=None, nrows=8, rowf=1024, desc=P, blocks=True):
    arr = (C.SampleJob * max(len(jobs), 1))(*jobs)
    out = ctypes.c_int(0)
    return L.cgl_sample_rows_dev_multi_prepare(len(jobs) if njobs is None else njobs, arr if jobs else None, nrows,
                                               rowf, desc, ctypes.byref(out) if blocks else None)


def test_sample_rows_multi_refusals():
    for over in (dict(desc=NUL), dict(desc=P4), dict(rnd=NUL), dict(blocks=0), dict(blocks=-8),
                 dict(blocks=(1 << 24) + 1)):
        assert _sample(**over) == E_ARG, over
    assert L.cgl_sample_rows_dev_multi_desc_bytes(0) == E_ARG
    assert L.cgl_sample_rows_dev_multi_desc_bytes(17) == E_ARG
    assert L.cgl_sample_rows_dev_multi_desc_bytes(16) > 0
    ok = [_job(), _job()]
    assert _sample_prepare([]) == E_ARG
    assert _sample_prepare(ok, njobs=17) == E_ARG
    assert _sample_prepare(ok, desc=NUL) == E_ARG
    assert _sample_prepare(ok, blocks=False) == E_ARG
    assert _sample_prepare(ok, nrows=0) == E_ARG
    assert _sample_prepare(ok, rowf=6) == E_ARG
    assert _sample_prepare(ok, rowf=0) == E_ARG
    assert _sample_prepare([_job(), _job(src=0)]) == E_ARG
    assert _sample_prepare([_job(), _job(dst=0)]) == E_ARG
    assert _sample_prepare([_job(), _job(src=4100)]) == E_ARG            # 16-byte rows
    assert _sample_prepare([_job(), _job(n_src=0)]) == E_ARG
    assert _sample_prepare([_job(), _job(nv=0, n_src=7)]) == E_ARG        # drop_last needs a whole batch


def _masks(desc=P, nm=24, blocks=24, rnd=P):
    return L.cgl_dropout2d_masks_dev_multi(desc, nm, blocks, rnd, 8, S)


def _mjob(mask=4096, n=16, c=32):
    j = C.MaskJob()
    j.mask, j.n, j.C, j.seed, j.counter = mask, n, c, 7, 3
    return j


def _masks_prepare(jobs, nm=None, p=0.25, desc=P, blocks=True):
    arr = (C.MaskJob * max(len(jobs), 1))(*jobs)
    out = ctypes.c_int(0)
    return L.cgl_dropout2d_masks_dev_multi_prepare(len(jobs) if nm is None else nm, arr if jobs else None, p, desc,
                                                   ctypes.byref(out) if blocks else None)


def test_dropout_masks_multi_refusals():
    for over in (dict(desc=NUL), dict(desc=P4), dict(rnd=NUL), dict(nm=0), dict(nm=129), dict(blocks=23),
                 dict(blocks=0)):
        assert _masks(**over) == E_ARG, over
    assert L.cgl_dropout2d_masks_dev_multi_desc_bytes(0) == E_ARG
    assert L.cgl_dropout2d_masks_dev_multi_desc_bytes(129) == E_ARG
    assert L.cgl_dropout2d_masks_dev_multi_desc_bytes(128) > 0
    ok = [_mjob(), _mjob()]
    assert _masks_prepare([]) == E_ARG
    assert _masks_prepare(ok, nm=129) == E_ARG
    assert _masks_prepare(ok, desc=NUL) == E_ARG
    assert _masks_prepare(ok, blocks=False) == E_ARG
    assert _masks_prepare(ok, p=1.0) == E_ARG
    assert _masks_prepare(ok, p=-0.1) == E_ARG
    assert _masks_prepare([_mjob(), _mjob(mask=0)]) == E_ARG
    assert _masks_prepare([_mjob(), _mjob(n=0)]) == E_ARG
    assert _masks_prepare([_mjob(), _mjob(c=0)]) == E_ARG


def test_grouped_ops_record_into_a_batch():
    """Inside an open batch the two grouped launches validate and record (one of each, on the batch's stream, beside
    the single forms); the _prepare calls, the broadcast and the grouped log launch are refused.  The batch is
    cancelled, so nothing recorded is launched."""
    other = ctypes.c_void_p(64)
    assert L.cgl_conv_batch_begin(S) == 0
    try:
        assert _sample(desc=NUL) == E_ARG                       # still validated
        assert L.cgl_sample_rows_dev_multi(P, 24, P, other) == E_ARG        # another stream
        assert _sample() == 0
        assert _sample() == E_ARG                               # one grouped sampler per batch
        assert L.cgl_sample_rows_dev(P, 20, 8, 1024, 1, P, P, P, S) == 0    # the single form keeps its own slot
        assert _masks(nm=129) == E_ARG
        assert L.cgl_dropout2d_masks_dev_multi(P, 24, 24, P, 8, other) == E_ARG
        assert _masks() == 0
        assert _masks() == E_ARG
        assert _sample_prepare([_job()]) == E_STATE
        assert _masks_prepare([_mjob()]) == E_STATE
        assert L.cgl_bcast_rows(P, 1024, P, 2048, 2, S) == E_STATE
        assert L.cgl_conv_round_log_group(ctypes.byref(_log_args()), 3, S) == E_STATE
    finally:
        assert L.cgl_conv_batch_cancel() == 0
    assert L.cgl_conv_batch_begin(S) == 0                       # a fresh batch starts empty
    assert L.cgl_conv_batch_end(S) == 0


@pytest.mark.parametrize("over", [dict(src=NUL), dict(dst=NUL), dict(src=P4), dict(dst=P4), dict(n=0), dict(n=6),
                                  dict(stride=1020), dict(stride=2050), dict(copies=0), dict(copies=17)])
def test_bcast_rows_refusals(over):
    a = dict(dict(src=P, n=1024, dst=P, stride=2048, copies=2), **over)
    assert L.cgl_bcast_rows(a["src"], a["n"], a["dst"], a["stride"], a["copies"], S) == E_ARG


def _log_args(**over):
    a = C.ConvRoundLogArgs()
    a.ring = a.lam_dev = a.lbuf = a.nv = a.losses_all = a.alpha_all = 4096
    a.counters = None
    a.n_workers, a.rank, a.weighting, a.half = 3, 0, 0, 0.5
    a.round, a.g_step, a.d_step = 1, 1, 1
    for k, v in over.items():
        setattr(a, k, v)
    return a


LOG_BAD = [dict(ring=None), dict(lam_dev=None), dict(lbuf=None), dict(nv=None), dict(losses_all=None),
           dict(alpha_all=None), dict(weighting=5), dict(weighting=-1), dict(n_workers=2), dict(n_workers=4),
           dict(rank=1), dict(round=0)]


@pytest.mark.parametrize("over", LOG_BAD)
def test_round_log_group_refusals(over):
    assert L.cgl_conv_round_log_group(ctypes.byref(_log_args(**over)), 3, S) == E_ARG


@pytest.mark.parametrize("workers", [0, 1, 17])
def test_round_log_group_worker_count(workers):
    assert L.cgl_conv_round_log_group(ctypes.byref(_log_args(n_workers=workers)), workers, S) == E_ARG
    assert L.cgl_conv_round_log_group(None, 3, S) == E_ARG


def test_defer_log_group_state():
    """The grouped record shares the deferral's one log slot with the single form; outside a deferral both are
    refused.  The deferral is cancelled: nothing recorded is launched."""
    ok = _log_args()
    assert L.cgl_conv_wgrad_defer_log_group(ctypes.byref(ok), 3) == E_STATE
    assert L.cgl_conv_wgrad_defer_begin() == 0
    try:
        for over in LOG_BAD:
            assert L.cgl_conv_wgrad_defer_log_group(ctypes.byref(_log_args(**over)), 3) == E_ARG, over
        assert L.cgl_conv_wgrad_defer_log_group(ctypes.byref(ok), 2) == E_ARG
        assert L.cgl_conv_wgrad_defer_log_group(ctypes.byref(ok), 3) == 0
        assert L.cgl_conv_wgrad_defer_log_group(ctypes.byref(ok), 3) == E_STATE
        assert L.cgl_conv_wgrad_defer_log(ctypes.byref(_log_args(n_workers=1))) == E_STATE
    finally:
        assert L.cgl_conv_wgrad_defer_cancel() == 0
    assert L.cgl_conv_wgrad_defer_begin() == 0
    try:
        assert L.cgl_conv_wgrad_defer_log(ctypes.byref(_log_args(n_workers=1))) == 0
        assert L.cgl_conv_wgrad_defer_log_group(ctypes.byref(ok), 3) == E_STATE
    finally:
        assert L.cgl_conv_wgrad_defer_cancel() == 0


def test_step_refusals_need_no_device():
    """The constructor's co-located refusals come before any allocation."""
    from cglgan.conv_step import ConvGanStep
    for kw in (dict(colocated=1), dict(colocated=17), dict(colocated=-2), dict(colocated=3, n_workers=2),
               dict(colocated=3, rank=1), dict(colocated=2, data=[None, None]), dict(colocated=2, data="x"),
               dict(colocated=2, gemm_dtype="f16")):
        with pytest.raises(ValueError):
            ConvGanStep(8, **kw)
