"""The tile cost model of the single-op / fused GEMM (gemm_cost and choose_tiles of csrc/cgl_runtime.hip),
restated in Python: the GEMM tests pick their shapes with it and check the library's choice against it."""
import math

OPTS = [(2, 2, 1), (2, 1, 2), (1, 2, 2), (1, 1, 4)]     # WM x WN x WK (choose_tiles' order)


def gemm_cost(M, N, K, WM, WN, WK, t):
    """gemm_cost of cgl_runtime.hip (unpacked operands: ta_a = ta_b = 1)"""
    tiles = -(-M // (32 * t * WM)) * -(-N // (32 * t * WN))
    wg_per_cu = math.ceil(tiles / 256.0)
    per = math.ceil(-(-K // 16) / WK)
    blk = 512.0 * t * t
    ta = wg_per_cu * 4 * per * (t + t) * 64.0
    return max(wg_per_cu * per * blk, per * max(blk, 2000.0 / 2), ta) + (400.0 * t * t if WK > 1 else 0.0)


def choose_tiles(M, N, K):
    """choose_tiles of cgl_runtime.hip: (t, WM, WN, WK) of the GEMM [M][N] over K"""
    best, sel = 1e300, None
    for t in (1, 2):
        for o in OPTS:
            c = gemm_cost(M, N, K, *o, t)
            if c < best * (1.0 - 1e-9):
                best, sel = c, (t,) + o
    return sel
