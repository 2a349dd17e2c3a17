"""Argument checks of the conv-path entry points, on the CPU: every call here must be refused on the host.

The library loads without a device, and an argument error returns before anything touches one (test_lib_exports.py
relies on the same).  Every case below is refused by a rule the header states or by the entry point's own check --
CGL_E_ARG (-1), CGL_E_STATE (-2) or CGL_E_SIZE (-3); no valid call is sent (it would reach the launch).  Pointers
that are only checked for null / alignment are the dummy address 4096.

cgl_bn2d_bwd_stats(colsum_part != null, C = 0) used to evaluate 256 % (C / 4) before C was validated and ended the
process with SIGFPE; its C = 0 case is part of the sweep below."""
import ctypes
import math

import pytest

from cglgan import _lib as C

L = C.lib
E_ARG, E_STATE, E_SIZE = -1, -2, -3
P = ctypes.c_void_p(4096)          # non-null, 256-byte aligned, never dereferenced
P4 = ctypes.c_void_p(4096 + 4)     # ... off by 4 bytes
NUL = ctypes.c_void_p(0)
S = ctypes.c_void_p(0)             # the null stream (never reached)
BIG = 1 << 40                      # a workspace size no check can find too small


def _bn_ws(n, hw, c, groups):
    b = L.cgl_bn2d_workspace_bytes(n, hw, c, groups)
    assert b > 0
    return b


# ---- cgl_bn2d_*: one valid argument set per entry point, one field made invalid per case --------------------------
BN_OK = dict(part=P, R=32, X=P, n=8, hw=16, C=64, groups=2, gamma=P, beta=P, rm=P, rv=P, train=1, act=0, Y=P, sm=P,
             si=P, scratch=NUL, coef=NUL, apply0=0, nv=NUL, ws=P, wsb=BIG, dY=P, post=NUL, post_out=NUL, drop=NUL,
             dX=P, dgamma=P, dbeta=P, pc=NUL, pld=0, colsum=NUL)


def _bn_call(entry, **over):
    a = dict(BN_OK, **over)
    if entry == "fwd":
        return L.cgl_bn2d_fwd(a["X"], a["n"], a["hw"], a["C"], a["groups"], a["gamma"], a["beta"], 0.8, 0.1, a["rm"],
                              a["rv"], a["train"], a["act"], 0.2, a["Y"], a["sm"], a["si"], a["nv"], a["ws"], a["wsb"],
                              S)
    if entry == "fwd_stats":
        return L.cgl_bn2d_fwd_stats(a["part"], a["R"], a["X"], a["n"], a["hw"], a["C"], a["groups"], a["gamma"],
                                    a["beta"], 0.8, 0.1, a["rm"], a["rv"], a["act"], 0.2, a["Y"], a["sm"], a["si"],
                                    a["scratch"], a["nv"], a["ws"], a["wsb"], S)
    if entry == "fwd_stats_coef":
        return L.cgl_bn2d_fwd_stats_coef(a["part"], a["R"], a["X"], a["n"], a["hw"], a["C"], a["groups"], a["gamma"],
                                         a["beta"], 0.8, 0.1, a["rm"], a["rv"], a["act"], 0.2, a["Y"], a["sm"],
                                         a["si"], a["scratch"], a["coef"], a["apply0"], a["nv"], a["ws"], a["wsb"], S)
    if entry == "bwd":
        return L.cgl_bn2d_bwd(a["dY"], a["post"], a["X"], a["n"], a["hw"], a["C"], a["groups"], a["sm"], a["si"],
                              a["gamma"], 0.2, a["post_out"], a["drop"], a["dX"], a["dgamma"], a["dbeta"], a["pc"],
                              a["pld"], a["nv"], a["ws"], a["wsb"], S)
    assert entry == "bwd_stats"
    return L.cgl_bn2d_bwd_stats(a["part"], a["R"], a["dY"], a["post"], a["X"], a["n"], a["hw"], a["C"], a["groups"],
                                a["sm"], a["si"], a["gamma"], 0.2, a["post_out"], a["drop"], a["dX"], a["dgamma"],
                                a["dbeta"], a["pc"], a["pld"], a["nv"], a["colsum"], a["ws"], a["wsb"], S)


BN_ENTRIES = ["fwd", "fwd_stats", "fwd_stats_coef", "bwd"]


@pytest.mark.parametrize("colsum", [False, True])
@pytest.mark.parametrize("c", [0, 1, 2, 3, 6, 512])
def test_bn2d_bwd_stats_channel_count(c, colsum):
    """C must be a power of two in 4 .. 256, with or without the column-sum partials.  (n hw = 256 here, so the
    colsum form's other conditions hold and C alone decides; C = 0 is the former SIGFPE.)"""
    assert _bn_call("bwd_stats", C=c, n=16, hw=16, colsum=P if colsum else NUL) == E_ARG


def test_bn2d_bwd_stats_colsum_rules():
    assert _bn_call("bwd_stats", n=8, hw=16, colsum=P) == E_ARG                   # n hw = 128: not whole 256-row chunks
    assert _bn_call("bwd_stats", n=16, hw=16, colsum=ctypes.c_void_p(4096 + 8)) == E_ARG    # 16-byte alignment
    assert _bn_call("bwd_stats", R=0) == E_ARG
    assert _bn_call("bwd_stats", R=48) == E_ARG                                   # gr = 64 rows per call
    assert _bn_call("bwd_stats", wsb=_bn_ws(8, 16, 64, 2) - 1) == E_SIZE
    assert _bn_call("bwd_stats", part=NUL) == E_ARG


@pytest.mark.parametrize("entry", BN_ENTRIES)
@pytest.mark.parametrize("field", ["n", "hw", "C", "groups"])
@pytest.mark.parametrize("bad", [0, -1])
def test_bn2d_sizes(entry, field, bad):
    assert _bn_call(entry, **{field: bad}) == E_ARG


@pytest.mark.parametrize("entry", BN_ENTRIES)
def test_bn2d_groups_and_buffers(entry):
    assert _bn_call(entry, n=8, groups=3) == E_ARG                                # n % groups != 0
    assert _bn_call(entry, wsb=_bn_ws(8, 16, 64, 2) - 1) == E_SIZE                # a workspace one byte short
    assert _bn_call(entry, ws=NUL) == E_ARG
    assert _bn_call(entry, X=P4) == E_ARG
    # only one of save_mean / save_invstd (the backward needs both)
    assert _bn_call(entry, sm=NUL) == E_ARG
    assert _bn_call(entry, si=NUL) == E_ARG
    if entry == "bwd":
        assert _bn_call(entry, pc=P, post=P) == E_ARG                             # post_coef replaces post
        assert _bn_call(entry, pc=P, groups=2) == E_ARG                           # ... for one forward call's rows
        return
    # only one of running_mean / running_var
    assert _bn_call(entry, rm=NUL) == E_ARG
    assert _bn_call(entry, rv=NUL) == E_ARG
    assert _bn_call(entry, act=2) == E_ARG
    if entry == "fwd":
        assert _bn_call(entry, train=0, rm=NUL, rv=NUL) == E_ARG                  # eval needs running statistics
        assert _bn_call(entry, n=1, hw=1, groups=1) == E_ARG                      # torch: more than 1 value per channel
        return
    assert _bn_call(entry, R=0) == E_ARG
    assert _bn_call(entry, R=-32) == E_ARG
    assert _bn_call(entry, R=48) == E_ARG                                         # gr = 4 * 16 = 64, 64 % 48 != 0
    assert _bn_call(entry, part=NUL) == E_ARG
    if entry == "fwd_stats_coef":
        assert _bn_call(entry, coef=P4) == E_ARG
        assert _bn_call(entry, apply0=-1) == E_ARG
        assert _bn_call(entry, apply0=9) == E_ARG


def test_bn2d_sizing_queries():
    for bad in (dict(n=0), dict(hw=0), dict(c=0), dict(groups=0), dict(n=8, groups=3)):
        a = dict(dict(n=8, hw=16, c=64, groups=2), **bad)
        assert L.cgl_bn2d_workspace_bytes(a["n"], a["hw"], a["c"], a["groups"]) == E_ARG
    assert L.cgl_bn2d_stats_scratch_bytes(0, 1) == E_ARG
    assert L.cgl_bn2d_stats_scratch_bytes(64, 0) == E_ARG


# ---- cgl_sample_rows_dev ----------------------------------------------------------------------------------------------
def _sample(src=P, n_src=100, nrows=8, rowf=1024, rd=P, dst=P, nv=P):
    return L.cgl_sample_rows_dev(src, n_src, nrows, rowf, 1234, rd, dst, nv, S)


def test_sample_rows_dev_args():
    assert _sample(n_src=0) == E_ARG
    assert _sample(nrows=0) == E_ARG
    for rowf in (0, 3, 6, -4):
        assert _sample(rowf=rowf) == E_ARG
    assert _sample(n_src=7, nrows=8, nv=NUL) == E_ARG        # drop_last has no whole batch when n_src < nrows
    assert _sample(src=P4) == E_ARG
    assert _sample(dst=P4) == E_ARG
    assert _sample(rd=NUL) == E_ARG
    assert _sample(src=NUL) == E_ARG
    assert _sample(dst=NUL) == E_ARG


# ---- cgl_dropout2d_mask(s)(_dev) -----------------------------------------------------------------------------------------
def _masks(nm=2, p=0.25, masks=None, n=None, c=None, dev=False, rd=P, null_lists=False):
    k = max(nm, 1)
    mp = (ctypes.c_void_p * k)(*(masks if masks is not None else [4096] * k))
    na = (ctypes.c_int * k)(*(n if n is not None else [4] * k))
    ca = (ctypes.c_int * k)(*(c if c is not None else [16] * k))
    ct = (ctypes.c_ulonglong * k)(*range(k))
    if null_lists:
        mp = None
    if dev:
        return L.cgl_dropout2d_masks_dev(nm, mp, na, ca, p, 1234, ct, rd, 1, S)
    return L.cgl_dropout2d_masks(nm, mp, na, ca, p, 1234, ct, S)


@pytest.mark.parametrize("p", [-0.1, 1.0, math.nan, math.inf, 1.5])
def test_dropout_probability(p):
    """p must lie in [0, 1): p = 1 would scale by 1 / 0, and NaN fails every comparison."""
    assert L.cgl_dropout2d_mask(P, 4, 16, p, 1, 0, S) == E_ARG
    assert _masks(p=p) == E_ARG
    assert _masks(p=p, dev=True) == E_ARG


def test_dropout_mask_lists():
    assert L.cgl_dropout2d_mask(NUL, 4, 16, 0.25, 1, 0, S) == E_ARG
    assert L.cgl_dropout2d_mask(P, 0, 16, 0.25, 1, 0, S) == E_ARG
    assert L.cgl_dropout2d_mask(P, 4, 0, 0.25, 1, 0, S) == E_ARG
    for dev in (False, True):
        assert _masks(nm=0, dev=dev) == E_ARG
        assert _masks(nm=17, dev=dev) == E_ARG               # at most 16 masks per launch
        assert _masks(nm=3, masks=[4096, 0, 4096], dev=dev) == E_ARG
        assert _masks(nm=3, n=[4, 0, 4], dev=dev) == E_ARG
        assert _masks(nm=3, c=[16, 16, -1], dev=dev) == E_ARG
        assert _masks(null_lists=True, dev=dev) == E_ARG
    assert _masks(dev=True, rd=NUL) == E_ARG


# ---- cgl_adam_multi(_dev) --------------------------------------------------------------------------------------------
def _adam(nt=2, step=1, ptrs=None, n=None, dev=False, sd=P, which="p"):
    k = max(nt, 1)
    full = (ctypes.c_void_p * k)(*([4096] * k))
    holed = (ctypes.c_void_p * k)(*(ptrs if ptrs is not None else [4096] * k))
    arrs = {w: (holed if w == which else full) for w in "pgmv"}
    ns = (ctypes.c_int64 * k)(*(n if n is not None else [8] * k))
    if dev:
        return L.cgl_adam_multi_dev(nt, arrs["p"], arrs["g"], arrs["m"], arrs["v"], ns, sd, 2e-4, 0.5, 0.999, 1e-8, S)
    return L.cgl_adam_multi(nt, arrs["p"], arrs["g"], arrs["m"], arrs["v"], ns, step, 2e-4, 0.5, 0.999, 1e-8, S)


def test_adam_multi_args():
    for dev in (False, True):
        assert _adam(nt=0, dev=dev) == E_ARG
        assert _adam(nt=33, dev=dev) == E_ARG                # at most 32 tensors per launch
        for which in "pgmv":                                 # a null entry of a non-empty tensor, in any list
            assert _adam(nt=3, ptrs=[4096, 0, 4096], dev=dev, which=which) == E_ARG
        assert _adam(nt=3, n=[8, -1, 8], dev=dev) == E_ARG
    assert _adam(step=0) == E_ARG                            # steps count from 1
    assert _adam(step=-3) == E_ARG
    assert _adam(dev=True, sd=NUL) == E_ARG
    # a list of empty tensors only: nothing to launch, and the null pointers torch gives empty tensors are accepted
    assert _adam(nt=2, ptrs=[0, 0], n=[0, 0]) == 0
    assert _adam(nt=2, ptrs=[0, 0], n=[0, 0], dev=True) == 0


# ---- cgl_adv_loss -------------------------------------------------------------------------------------------------------
def test_adv_loss_args():
    def call(x=P, M=8, Cc=1, loss=2, target=0):
        return L.cgl_adv_loss(x, M, Cc, loss, target, 1.0, P, P, NUL, S)
    assert call(loss=-1) == E_ARG
    assert call(loss=4) == E_ARG
    assert call(target=2) == E_ARG
    assert call(target=-1) == E_ARG
    assert call(loss=0, Cc=1) == E_ARG                       # CrossEntropy needs the two logits
    for loss in (1, 2, 3):
        assert call(loss=loss, Cc=2) == E_ARG                # ... and the one-column losses exactly one
    assert call(loss=0, Cc=3) == E_ARG
    assert call(M=0) == E_ARG
    assert call(M=-5) == E_ARG
    assert call(x=NUL) == E_ARG


# ---- cgl_dense1_head_nhwc ------------------------------------------------------------------------------------------------
def _head(n=8, c=128, hw=4, loss=2, n0=4, t0=1, t1=0, coef=NUL, in_groups=1, scratch=P, W=P, dX=P):
    return L.cgl_dense1_head_nhwc(P, W, P, P, NUL, P, dX, n, c, hw, loss, n0, t0, 0.5, P, NUL, t1, 0.5, P, coef,
                                  in_groups, scratch, S)


def test_dense1_head_args():
    for c in (0, 2, 6):
        assert _head(c=c) == E_ARG
    assert _head(c=32, hw=4) == E_ARG                        # c hw = 128: not a multiple of 256
    assert _head(c=128, hw=10) == E_ARG                      # c hw = 1280 > 1024
    assert _head(n0=0) == E_ARG
    assert _head(n0=9) == E_ARG                              # n + 1
    assert _head(loss=0) == E_ARG                            # one logit: no CrossEntropy head
    assert _head(loss=4) == E_ARG
    assert _head(coef=P, in_groups=0) == E_ARG
    assert _head(coef=P, in_groups=3) == E_ARG               # n % in_groups != 0
    assert _head(t0=2) == E_ARG
    assert _head(t1=2) == E_ARG                              # (a second call exists: n0 < n)
    assert _head(scratch=NUL) == E_ARG
    assert _head(n=0, n0=0) == E_ARG
    assert _head(W=P4) == E_ARG
    assert _head(dX=P4) == E_ARG
    assert L.cgl_dense1_fwd_nhwc(P, P, P, P, NUL, 8, 32, 4, S) == E_ARG
    assert L.cgl_dense1_bwd_data_nhwc(P, P, P, 8, 6, 4, S) == E_ARG


# ---- cgl_gather_rows, cgl_colsum_finalize, layout changes --------------------------------------------------------------------
def test_gather_colsum_layout_args():
    assert L.cgl_gather_rows(P, NUL, 0, -1, 4, P, S) == E_ARG
    assert L.cgl_gather_rows(P, NUL, 0, 8, 0, P, S) == E_ARG
    assert L.cgl_gather_rows(P, NUL, -1, 8, 4, P, S) == E_ARG
    assert L.cgl_gather_rows(NUL, NUL, 0, 8, 4, P, S) == E_ARG
    assert L.cgl_gather_rows(P, NUL, 0, 0, 4, P, S) == 0     # no rows: nothing to launch
    assert L.cgl_colsum_finalize(P, 0, 64, P, S) == E_ARG
    assert L.cgl_colsum_finalize(P, 4, 0, P, S) == E_ARG
    assert L.cgl_colsum_finalize(NUL, 4, 64, P, S) == E_ARG
    for fn in (L.cgl_nchw_to_nhwc, L.cgl_nhwc_to_nchw):
        assert fn(P, P, 0, 4, 4, S) == E_ARG
        assert fn(P, P, 2, 0, 4, S) == E_ARG
        assert fn(P, P, 2, 4, 0, S) == E_ARG
        assert fn(NUL, P, 2, 4, 4, S) == E_ARG


# ---- cgl_conv3x3_*: the geometry rules shared by every variant -------------------------------------------------------------
GEOM_BAD = [dict(stride=0), dict(stride=3), dict(up=1, stride=2), dict(cin=0), dict(cout=0), dict(n=0), dict(h=0),
            dict(up=2), dict(cin=65537)]


@pytest.mark.parametrize("bad", GEOM_BAD, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_conv3x3_geometry(bad):
    g = dict(dict(n=2, h=8, w=8, cin=16, cout=32, stride=1, up=0), **bad)
    geo = (g["n"], g["h"], g["w"], g["cin"], g["cout"], g["stride"], g["up"])
    assert L.cgl_conv3x3_workspace_bytes(*geo) < 0
    assert L.cgl_conv3x3_fwd(P, P, P, P, *geo, 0, 0.2, NUL, P, BIG, S) == E_ARG
    assert L.cgl_conv3x3_bwd_data(P, P, P, *geo, P, BIG, S) == E_ARG
    assert L.cgl_conv3x3_bwd_weight(P, P, P, P, *geo, P, BIG, S) == E_ARG
    assert L.cgl_conv3x3_fwd_packed(P, P, P, P, *geo, 0, 0.2, NUL, P, BIG, S) == E_ARG
    assert L.cgl_conv3x3_bwd_data_packed(P, P, P, P, *geo, P, BIG, S) == E_ARG
    assert L.cgl_conv3x3_fwd_packed_stats(P, P, P, P, *geo, 0, 0.2, NUL, 1, P, NUL, P, BIG, S) == E_ARG
    assert L.cgl_conv3x3_stat_chunks(*geo, 1) < 0
    assert L.cgl_conv3x3_bias_by_colsum(*geo) < 0


def test_batch_state():
    """While a launch batch is open the other launching entry points return CGL_E_STATE before looking at their
    arguments; the batch is closed empty (nothing recorded, nothing launched)."""
    assert L.cgl_conv_batch_begin(S) == 0
    try:
        assert _bn_call("fwd") == E_STATE
        assert _bn_call("bwd_stats", C=0, colsum=P) == E_STATE
        assert L.cgl_gather_rows(P, NUL, 0, 8, 4, P, S) == E_STATE
        assert L.cgl_colsum_finalize(P, 4, 64, P, S) == E_STATE
        assert _adam() == E_STATE
        assert _head() == E_STATE
        # the calls a batch records still validate first
        assert _sample(rowf=3) == E_ARG
        assert _masks(nm=17) == E_ARG
        assert L.cgl_adv_loss(P, 0, 1, 2, 0, 1.0, P, P, NUL, S) == E_ARG
    finally:
        assert L.cgl_conv_batch_end(S) == 0
