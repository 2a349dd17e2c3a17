"""What the GEMM's tile cost model can select (CPU only; the GPU side is tests/test_gpu_ops.py)."""
import itertools

from gemm_tile_model import OPTS, choose_tiles


def test_tile_model_reach():
    """What choose_tiles can select, from the restated cost model alone (no GPU work).

    t = 2 (tm = 2) is NEVER selected by an unforced choose_tiles, at any size: against the same arrangement with
    t = 1 it has at most 4x fewer tiles, so w = ceil(tiles / 256) shrinks at most 4x, while the per-workgroup MFMA
    work (512 t^2) grows 4x: the MFMA term w per 512 t^2 does not fall.  The chain term per max(512 t^2, 1000) and
    the split-K term 400 t^2 grow, and at t = 1 the load term (w 4 per 2 t 64 = 512 w per) equals the MFMA term, so
    it never decides.  The t = 2 cost is therefore never strictly below the t = 1 cost of the same arrangement, and
    ties keep the earlier candidate (t = 1).  (tm = 2 is reached only by the fused step's plan, which forces it.)
    The search below confirms it for every tile class up to 1056 per dimension and every depth up to 1040, and
    that the other four arrangements are all selectable there; cgl_gemm_f32_arg<2, 2> is therefore unreachable
    through cgl_linear_prepare / cgl_linear_* and has no case in the sweep."""
    found = {}
    for mi, ni, nch in itertools.product(range(1, 34), range(1, 34), range(1, 66)):
        found.setdefault(choose_tiles(32 * mi, 32 * ni, 16 * nch), (32 * mi, 32 * ni, 16 * nch))
    assert set(found) == {(1,) + o for o in OPTS}, found
    for Mg, Ng, Kg in ((4096, 4096, 16), (8192, 8192, 4096), (100000, 64, 64), (64, 100000, 1 << 20)):
        assert choose_tiles(Mg, Ng, Kg)[0] == 1
