"""Single HIP ops vs plain PyTorch fp32 on the GPU (the kernels under the fused step).

Tolerance: fp32 MFMA is an exact k-ordered fma chain; only the summation order differs from
torch's GEMM, so <= 1e-5 relative (norm) is required.

A norm cannot see one wrong element of a 512 x 1024 output, so every GEMM result is also held, element by
element, to the worst-case bound of an fp32 dot product in ANY summation order against the fp64 product of the
same fp32 operands (computed on the CPU):  |C - C64| <= (K + 8) u (|A| |B|^T + |bias|),  u = 2^-24  (Higham,
Accuracy and Stability of Numerical Algorithms, section 3.1: gamma_K ~ K u; the 8 covers the bias add, the
LeakyReLU multiply and the split-K partial sums).  A dropped or doubled k term breaks it by orders of magnitude.
Tanh / Sigmoid are 1-Lipschitz and evaluated within 2 u: + 2 u.  LeakyReLU is 1-Lipschitz too, so the bound
holds across its kink; the new cases still take their seed away from it (parity_helpers.KINK_MARGIN).

The sweep (SWEEP below) is chosen with a restatement of the library's tile cost model (gemm_cost /
choose_tiles of cgl_runtime.hip: tests/gemm_tile_model.py) so that every wave arrangement the model can select is run:
test_linear_tile_coverage decodes the arrangement of every swept case from what cgl_linear_prepare reports.
"""
import ctypes
import itertools
import math

import pytest
import torch

from cglgan import _lib as C
from gemm_tile_model import OPTS, choose_tiles as _choose_tiles

pytestmark = pytest.mark.gpu
TOL = 1e-5


def _rel(a, b):
    return float((a.double() - b.double()).norm() / max(b.double().norm(), 1e-30))


def _ws():
    return torch.zeros(C.lib.cgl_op_workspace_bytes(), dtype=torch.uint8, device="cuda")


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


U = 2.0 ** -24


def _elementwise(got, ref64, bound, what):
    """|got - ref64| <= bound, element by element (fp64, on the CPU); prints the worst ratio."""
    got = got.detach().double().cpu().reshape(ref64.shape)
    assert torch.isfinite(got).all(), what
    ratio = ((got - ref64).abs() / bound.clamp_min(1e-300))
    worst = float(ratio.max())
    print(f"{what}: worst |err| / bound {worst:.4f}")
    assert worst <= 1.0, f"{what}: element {int(ratio.argmax())} is {worst:.3g} x the elementwise bound"
    return worst


def _ref_fwd(X, W, b, act, slope=0.2):
    """fp64 act(X W^T + b) of the fp32 operands and its elementwise bound (K + 8) u (|X| |W|^T + |b|) [+ 2 u]"""
    K = X.shape[1]
    X, W = X.double(), W.double()
    ref = X @ W.t()
    mag = X.abs() @ W.abs().t()
    if b is not None:
        ref, mag = ref + b.double(), mag + b.double().abs()
    bound = (K + 8) * U * mag
    if act == 1:
        ref = torch.where(ref > 0, ref, ref * float(torch.tensor(slope, dtype=torch.float32)))
    elif act == 2:
        ref, bound = torch.tanh(ref), bound + 2 * U
    elif act == 3:
        ref, bound = torch.sigmoid(ref), bound + 2 * U
    return ref, bound


def _ref_bwd_data(dY, W):
    N = dY.shape[1]
    return dY.double() @ W.double(), (N + 8) * U * (dY.double().abs() @ W.double().abs())


def _ref_bwd_weight(dY, X):
    M = dY.shape[0]
    dY, X = dY.double(), X.double()
    return ((dY.t() @ X, (M + 8) * U * (dY.abs().t() @ X.abs())), (dY.sum(0), (M + 8) * U * dY.abs().sum(0)))


SHAPES = [(256, 128, 100), (512, 784, 1024), (37, 50, 100), (1, 2, 256), (300, 33, 2), (64, 1, 32), (512, 1024, 512)]


@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("act", [0, 1, 2])
def test_linear_fwd(M, N, K, act):
    g = torch.Generator(device="cuda").manual_seed(M * 7 + N + K)
    X = torch.randn(M, K, device="cuda", generator=g)
    W = torch.randn(N, K, device="cuda", generator=g) * 0.05
    b = torch.randn(N, device="cuda", generator=g)
    Y = torch.empty(M, N, device="cuda")
    ws = _ws()
    C.check(C.lib.cgl_linear_fwd(_p(X), _p(W), _p(b), _p(Y), M, N, K, act, 0.2, _p(ws), ws.numel(), _s()))
    ref = torch.nn.functional.linear(X, W, b)
    ref = [ref, torch.nn.functional.leaky_relu(ref, 0.2), torch.tanh(ref)][act]
    assert _rel(Y, ref) <= TOL
    ref64, bound = _ref_fwd(X.cpu(), W.cpu(), b.cpu(), act)
    _elementwise(Y, ref64, bound, f"linear_fwd {M}x{N}x{K} act={act}")


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_linear_bwd(M, N, K):
    g = torch.Generator(device="cuda").manual_seed(M + 3 * N + K)
    X = torch.randn(M, K, device="cuda", generator=g)
    W = torch.randn(N, K, device="cuda", generator=g) * 0.05
    dY = torch.randn(M, N, device="cuda", generator=g)
    dX = torch.empty(M, K, device="cuda")
    dW = torch.empty(N, K, device="cuda")
    db = torch.empty(N, device="cuda")
    ws = _ws()
    C.check(C.lib.cgl_linear_bwd_data(_p(dY), _p(W), _p(dX), M, N, K, _p(ws), ws.numel(), _s()))
    C.check(C.lib.cgl_linear_bwd_weight(_p(dY), _p(X), _p(dW), _p(db), M, N, K, _p(ws), ws.numel(), _s()))
    assert _rel(dX, dY @ W) <= TOL
    assert _rel(dW, dY.t() @ X) <= TOL
    assert _rel(db, dY.sum(0)) <= TOL
    ref64, bound = _ref_bwd_data(dY.cpu(), W.cpu())
    _elementwise(dX, ref64, bound, f"linear_bwd_data {M}x{N}x{K}")
    (rw, bw), (rb, bb) = _ref_bwd_weight(dY.cpu(), X.cpu())
    _elementwise(dW, rw, bw, f"linear_bwd_weight {M}x{N}x{K} dW")
    _elementwise(db, rb, bb, f"linear_bwd_weight {M}x{N}x{K} db")


def test_adam_matches_torch_single_tensor():
    from oracle.gan_oracle import Adam
    n = 100003
    g = torch.Generator().manual_seed(1)
    p0 = torch.randn(n, generator=g)
    ref_p = p0.clone().requires_grad_(True)
    opt = Adam([ref_p])
    p, m, v = p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    ws = _ws()
    for t in range(1, 6):
        grad = torch.randn(n, generator=g)
        ref_p.grad = grad.clone()
        opt.step()
        gd = grad.cuda()
        C.check(C.lib.cgl_adam_step(_p(p), _p(gd), _p(m), _p(v), n, t, 2e-4, 0.5, 0.999, 1e-8, _p(ws), ws.numel(),
                                    _s()))
    torch.cuda.synchronize()
    assert _rel(p.cpu(), ref_p.detach()) <= 1e-6
    assert _rel(m.cpu(), opt.m[0]) <= 1e-6
    assert _rel(v.cpu(), opt.v[0]) <= 1e-6


def test_normal_fill_moments():
    n = 1 << 20
    out = torch.empty(n, device="cuda")
    C.check(C.lib.cgl_normal_fill(_p(out), n, 1234, 0, 0, _s()))
    torch.cuda.synchronize()
    assert abs(out.mean().item()) < 5e-3
    assert abs(out.std().item() - 1.0) < 5e-3
    out2 = torch.empty(n, device="cuda")
    C.check(C.lib.cgl_normal_fill(_p(out2), n, 1234, 0, 0, _s()))
    torch.cuda.synchronize()
    assert torch.equal(out, out2)


# ---------------------------------------------------------------------------------------------------
# The single-op GEMM at its edges: a shape sweep that reaches every code path of cgl_gemm_f32_arg that
# choose_tiles can select, by value (cgl_linear_fwd / _bwd_data / _bwd_weight) and prepared
# (cgl_linear_prepare + cgl_linear_launch), every output carved from a sentinel-filled buffer.
KINK_MARGIN = 1e-6    # parity_helpers.KINK_MARGIN: min |LeakyReLU input| / std
PAD = 64              # sentinel words on either side of an output
SENTINEL = -12345.625
def _gemm_dims(op, M, N, K, db=True):
    """the GEMM (rows, columns, depth) behind Linear op 0 / 1 / 2 of an [M, K] x [N, K] layer (make_gemm calls)"""
    return [(M, N, K), (M, K, N), (N, K + (1 if db else 0), M)][op]


def _decode(launch, Mg, Ng):
    """every (t, WM, WN, WK) consistent with what cgl_linear_prepare reported: shmem = WM WN (WK - 1) t^2 4096
    bytes, grid = tiles_m tiles_n (the two WK = 2 orientations can coincide; then both are returned)"""
    t = launch.tm
    return [(t,) + o for o in OPTS
            if o[0] * o[1] * (o[2] - 1) * t * t * 4096 == launch.shmem
            and -(-Mg // (32 * t * o[0])) * -(-Ng // (32 * t * o[1])) == launch.grid]


def _layer(op, a, b, k):
    """Linear (M, N, K) whose op has output a x b and contraction length k"""
    return [(a, b, k), (a, k, b), (k, a, b)][op]


_DIMS = [31, 32, 33, 65, 129, 257]
_KS = [1, 3, 15, 16, 17, 33, 47, 100, 257]
# the cross of the two output dimensions with K, thinned to a Latin selection (54 of 324: every (dim, dim),
# (dim, K) pair of values still occurs; 257 x 257 x 257 is in it)
_SWEEP_ABK = [(a, b, k) for (ia, a), (ib, b), (ik, k) in itertools.product(enumerate(_DIMS), enumerate(_DIMS),
                                                                         enumerate(_KS)) if (ia + ib + ik) % 6 == 0]
# + the one arrangement the thinned cross does not reach, 1 x 2 x 2 (chosen when it needs one wave of
# workgroups and 2 x 1 x 2 needs two: 17 x 15 = 255 tiles against 9 x 29 = 261), found with _choose_tiles
_EXTRA_ABK = [(513, 897, 17)]
SWEEP = [(op,) + abk for op in range(3) for abk in _SWEEP_ABK + _EXTRA_ABK]


def _operand(shape, g, scale=1.0, misaligned=False):
    """fp32 CPU values and their device copy; misaligned: contiguous, but starting 4 bytes off a 16-byte boundary"""
    n = math.prod(shape)
    cpu = torch.randn(shape, generator=g) * scale
    if misaligned:
        dev = torch.empty(n + 1, device="cuda")[1:].view(shape)
        assert dev.data_ptr() % 16 == 4
    else:
        dev = torch.empty(shape, device="cuda")
        assert dev.data_ptr() % 16 == 0
    dev.copy_(cpu)
    return cpu, dev


def _sentinel_out(shape):
    n = math.prod(shape)
    buf = torch.full((PAD + n + PAD,), SENTINEL, device="cuda")
    return buf, buf[PAD:PAD + n].view(shape)


def _sentinel_ok(buf, what):
    n = buf.numel() - 2 * PAD
    assert (buf[:PAD] == SENTINEL).all() and (buf[PAD + n:] == SENTINEL).all(), f"{what}: stores outside the output"


def _run_linear(op, M, N, K, act=0, bias=True, db=True, mis_a=False, mis_b=False, seed=0):
    """One Linear op by value and prepared; checks both against the fp64 reference (elementwise), against each
    other (bitwise) and the sentinels; returns the CglLinearLaunch of the prepared form."""
    from cglgan import conv_ops
    what = f"op{op} {M}x{N}x{K} act={act} bias={bias} db={db} mis=({int(mis_a)},{int(mis_b)})"
    ws = _ws()
    for sd in range(seed, seed + 64):
        g = torch.Generator().manual_seed(1000003 * op + 7919 * M + 104729 * N + K + sd)
        if op == 0:
            (Ac, A), (Bc, B) = _operand((M, K), g, 1.0, mis_a), _operand((N, K), g, 0.05, mis_b)
            bc = torch.randn(N, generator=g) if bias else None
            ref, bound = _ref_fwd(Ac, Bc, bc, act)
            if act == 1:
                pre, _ = _ref_fwd(Ac, Bc, bc, 0)
                if float(pre.abs().min()) < KINK_MARGIN * float(pre.std() if pre.numel() > 1 else 1.0):
                    continue
        elif op == 1:
            (Ac, A), (Bc, B) = _operand((M, N), g, 1.0, mis_a), _operand((N, K), g, 0.05, mis_b)
            ref, bound = _ref_bwd_data(Ac, Bc)
        else:
            (Ac, A), (Bc, B) = _operand((M, N), g, 1.0, mis_a), _operand((M, K), g, 1.0, mis_b)
            (ref, bound), (ref_db, bound_db) = _ref_bwd_weight(Ac, Bc)
        break
    else:
        raise RuntimeError("no well-conditioned seed found")
    oshape = [(M, N), (M, K), (N, K)][op]
    outs = []
    for prepared in (False, True):
        cbuf, Cout = _sentinel_out(oshape)
        dbuf, dbo = _sentinel_out((N,)) if (op == 2 and db) else (None, None)
        bd = bc.cuda() if (op == 0 and bias) else None
        if prepared:
            pl = conv_ops.PreparedLinear(op, A, B, bd, Cout, dbo, M, N, K, act=act, slope=0.2)
            pl()
        elif op == 0:
            C.check(C.lib.cgl_linear_fwd(_p(A), _p(B), _p(bd), _p(Cout), M, N, K, act, 0.2, _p(ws), ws.numel(), _s()))
        elif op == 1:
            C.check(C.lib.cgl_linear_bwd_data(_p(A), _p(B), _p(Cout), M, N, K, _p(ws), ws.numel(), _s()))
        else:
            C.check(C.lib.cgl_linear_bwd_weight(_p(A), _p(B), _p(Cout), _p(dbo), M, N, K, _p(ws), ws.numel(), _s()))
        torch.cuda.synchronize()
        tag = what + (" prepared" if prepared else " by value")
        _sentinel_ok(cbuf, tag)
        _elementwise(Cout, ref, bound, tag)
        if dbo is not None:
            _sentinel_ok(dbuf, tag + " db")
            _elementwise(dbo, ref_db, bound_db, tag + " db")
        outs.append((Cout, dbo))
    # both entry points run cgl_gemm_body with the same descriptor fields
    assert torch.equal(outs[0][0], outs[1][0]), what + ": prepared differs from by-value"
    if outs[0][1] is not None:
        assert torch.equal(outs[0][1], outs[1][1]), what + ": prepared db differs from by-value"
    Mg, Ng, Kg = _gemm_dims(op, M, N, K, db)
    assert _choose_tiles(Mg, Ng, Kg) in _decode(pl.launch, Mg, Ng), \
        f"{what}: the library chose {_decode(pl.launch, Mg, Ng)}, the restated cost model {_choose_tiles(Mg, Ng, Kg)}"
    return pl.launch


@pytest.mark.parametrize("op,a,b,k", SWEEP)
def test_linear_sweep(op, a, b, k):
    """Worst |err| / bound measured on the MI355X over the sweep: op 0 0.25, op 1 0.19, op 2 0.23 (db 0.12); the
    prepared form is bitwise the by-value form at every case."""
    _run_linear(op, *_layer(op, a, b, k))


@pytest.mark.parametrize("act", [1, 2, 3])
@pytest.mark.parametrize("M,N,K", [(65, 33, 100), (129, 257, 17), (33, 65, 3)])
def test_linear_fwd_activations(M, N, K, act):
    """op 0 with LeakyReLU / Tanh / Sigmoid (act = 3 is accepted by cgl_linear_fwd and was never run)"""
    _run_linear(0, M, N, K, act=act)


@pytest.mark.parametrize("M,N,K", [(33, 65, 47), (65, 31, 16), (257, 129, 100)])
def test_linear_null_bias_and_db(M, N, K):
    """bias = NULL (op 0) and db = NULL (op 2: no ones-column, the GEMM is [N][K], not [N][K + 1])"""
    _run_linear(0, M, N, K, bias=False)
    _run_linear(0, M, N, K, act=3, bias=False)
    _run_linear(2, M, N, K, db=False)


@pytest.mark.parametrize("mis_a,mis_b", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("op", [0, 1, 2])
@pytest.mark.parametrize("M,N,K", [(36, 68, 100), (132, 36, 16)])
def test_linear_misaligned_operands(M, N, K, op, mis_a, mis_b):
    """Contiguous operands that start 4 bytes off a 16-byte boundary (every dimension a multiple of 4, so only
    the address turns the 16-byte loads off -- set_vec, for that operand alone)"""
    _run_linear(op, M, N, K, mis_a=mis_a, mis_b=mis_b)


def test_linear_tile_coverage():
    """Across the sweep, per layout (op 0, 1, 2), cgl_linear_prepare selects WK in {1, 2, 4}, both orientations
    of the WK = 2 split (2 x 1 x 2 and 1 x 2 x 2) and 2 x 2 x 1 -- decoded from the reported tm / grid / shmem
    alone, counting a case only where the decode is unambiguous -- and at least one case has fewer 16-chunks of
    K than WK wave groups (so some groups get no chunk).  Reached on the MI355X, for each of the three layouts:
    (t, WM x WN x WK) = (1, 2x2x1), (1, 2x1x2), (1, 1x2x2), (1, 1x1x4); fewer chunks than WK e.g. at K = 33 and 47
    (3 chunks, WK = 4).  Missing: every t = 2 arrangement -- tm = 2 cannot be selected through these entry points
    at any size (argument and search: tests/test_gemm_tile_model.py), so it is listed here and not forced."""
    lib_ops = C.lib
    dummy = torch.zeros(1024 * 1024 + 16, device="cuda")
    desc = torch.zeros(int(lib_ops.cgl_linear_desc_bytes()), dtype=torch.uint8, device="cuda")
    for op in range(3):
        reached, starved = set(), []
        for _, a, b, k in [c for c in SWEEP if c[0] == op]:
            M, N, K = _layer(op, a, b, k)
            launch = C.LinearLaunch()
            C.check(lib_ops.cgl_linear_prepare(op, _p(dummy), _p(dummy), None, _p(dummy),
                                               _p(dummy) if op == 2 else None, M, N, K, 0, 0.2, _p(desc),
                                               ctypes.byref(launch)))
            Mg, Ng, Kg = _gemm_dims(op, M, N, K)
            cand = _decode(launch, Mg, Ng)
            assert cand, (f"op{op} {M}x{N}x{K}: tm={launch.tm} grid={launch.grid} shmem={launch.shmem} "
                          "decodes to nothing")
            assert _choose_tiles(Mg, Ng, Kg) in cand
            if len(cand) == 1:
                reached.add(cand[0])
                if -(-Kg // 16) < cand[0][3]:
                    starved.append((M, N, K))
        print(f"op{op}: reached (t, WM, WN, WK) = {sorted(reached)}; fewer chunks than WK at {starved[:4]}")
        assert reached == {(1,) + o for o in OPTS}, f"op{op}: reached only {sorted(reached)}"
        assert starved, f"op{op}: no case with fewer 16-chunks than WK"
