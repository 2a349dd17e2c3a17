"""Co-located workers, host side (no GPU): what cgl_gan_workspace_bytes accepts and refuses for
cgl_gan_config.colocated, the driver's ``colocate`` limits, and where ``ColocatedExchange`` cuts its launches."""
import ctypes
import types

import pytest

from cglgan import _lib as C
from cglgan import specs
from cglgan.driver import DriverConfig
from cglgan.exchange import ColocatedExchange
from cglgan.step import _spec


def _cfg(W, n_workers=None, rank=0, exchange_layer=-1, loss_scale=0.0, gemm_dtype=C.DTYPE_F32):
    cfg = C.GanConfig()
    cfg.g, cfg.d = _spec(specs.mnist_generator()), _spec(specs.mnist_discriminator())
    cfg.batch, cfg.batch_real, cfg.epoch = 64, 64, 1
    cfg.loss, cfg.weighting = C.LOSS_CE2, C.WEIGHT_CAPGAN
    cfg.n_workers, cfg.rank, cfg.exchange_layer = (W if n_workers is None else n_workers), rank, exchange_layer
    cfg.lr_g = cfg.lr_d = 2e-4
    cfg.beta1, cfg.beta2, cfg.adam_eps = 0.5, 0.999, 1e-8
    cfg.bn_eps, cfg.bn_momentum, cfg.slope = 0.8, 0.1, 0.2
    cfg.seed, cfg.gemm_dtype, cfg.loss_scale = 1, gemm_dtype, loss_scale
    cfg.colocated = W
    return cfg


def _ws(cfg):
    return C.lib.cgl_gan_workspace_bytes(ctypes.byref(cfg))


def test_workspace_accepts_two_workers_and_the_cap():
    assert _ws(_cfg(2)) > 0
    assert _ws(_cfg(C.MAX_COLOCATED)) > 0
    assert C.MAX_COLOCATED == 16


def test_workspace_grows_with_the_workers():
    one = _cfg(0, n_workers=1)
    assert _ws(_cfg(4)) > _ws(_cfg(2)) > _ws(one) > 0
    # colocated = 1 is "off": the one-worker carve
    assert _ws(_cfg(1, n_workers=1)) == _ws(one)


@pytest.mark.parametrize("cfg", [
    _cfg(C.MAX_COLOCATED + 1),                       # above the cap
    _cfg(3, n_workers=2),                            # n_workers != W
    _cfg(3, n_workers=1),
    _cfg(3, rank=1),                                 # rank != 0
    _cfg(3, exchange_layer=2),                       # Mix-G trunk / head split
    _cfg(3, loss_scale=65536.0, gemm_dtype=C.DTYPE_BF16),   # loss scaling
    _cfg(-1, n_workers=1),
], ids=["above_cap", "n_workers_2", "n_workers_1", "rank_1", "exchange_layer", "loss_scale", "negative"])
def test_workspace_refuses(cfg):
    assert _ws(cfg) == -1      # CGL_E_ARG


def test_loss_scale_config_is_valid_without_colocation():
    """The refused loss-scale configuration above is refused for the co-location, not for itself."""
    assert _ws(_cfg(0, n_workers=1, loss_scale=65536.0, gemm_dtype=C.DTYPE_BF16)) > 0


def test_every_dtype_and_weighting_allowed():
    for dt in (C.DTYPE_F32, C.DTYPE_F16, C.DTYPE_BF16):
        assert _ws(_cfg(3, gemm_dtype=dt)) > 0
    for wt in range(5):
        cfg = _cfg(3)
        cfg.weighting = wt
        assert _ws(cfg) > 0


def test_driver_config_limits():
    with pytest.raises(ValueError, match="mixg"):
        DriverConfig(colocate=True, algo="mixg", num_workers=4).validate()
    with pytest.raises(ValueError, match="num_servers"):
        DriverConfig(colocate=True, num_servers=2, num_workers=4).validate()
    assert DriverConfig(colocate=True, num_workers=10).validate().colocate
    assert DriverConfig(colocate=True, algo="mdgan", num_workers=3).validate().colocate
    assert DriverConfig().colocate is False


def test_driver_colocate_needs_world_one():
    from cglgan.driver import Driver
    with pytest.raises(ValueError, match="world size"):
        Driver(DriverConfig(colocate=True, num_workers=3, dataset_rows=600), rank=0, world=3)
    # without the flag nothing changes: one process per worker
    with pytest.raises(ValueError, match="one process per worker"):
        Driver(DriverConfig(num_workers=3, dataset_rows=600), rank=0, world=1)


def _exchange(W, share, swap):
    return ColocatedExchange(types.SimpleNamespace(colocated=W), share_every=share, swap_every=swap)


def test_exchange_chunks_cut_at_share_and_swap():
    ex = _exchange(3, 2, 3)
    # rounds 0..5: share after rounds 1, 3, 5; swap after rounds 2, 5
    assert ex.chunks(0, 6) == [2, 1, 1, 2]
    assert ex.chunks(0, 4) == [2, 1, 1]
    assert ex.chunks(4, 2) == [2]
    assert ex.chunks(1, 4) == [1, 1, 1, 1]
    for r0 in range(7):
        for n in range(0, 15):
            ch = ex.chunks(r0, n)
            assert sum(ch) == n and all(m >= 1 for m in ch)
            # a share / swap round is always the last of its launch
            r = r0
            for m in ch:
                assert not any(any(ex._due(q)) for q in range(r, r + m - 1))
                r += m
    assert _exchange(2, 0, 0).chunks(3, 10) == [10]
    assert _exchange(2, 1, 0).chunks(0, 3) == [1, 1, 1]


def test_exchange_needs_a_colocated_step():
    with pytest.raises(ValueError):
        ColocatedExchange(types.SimpleNamespace(colocated=0))
