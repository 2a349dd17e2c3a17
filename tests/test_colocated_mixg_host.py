"""Co-located Mix-G / CGLGAN, host side (no GPU): what cgl_gan_config.colocated_heads accepts and refuses, the
[trunk | head 0 | ... | head W-1] layout the layout queries report, and the group specs' state-dict keys."""
import ctypes

import pytest

from cglgan import _lib as C
from cglgan import specs
from cglgan.step import _spec

XL = specs.MIXGEN_HEAD_LAYER


def _cfg(W, heads=1, exchange_layer=XL, loss_scale=0.0, gemm_dtype=C.DTYPE_F32, g=None, d=None, loss=C.LOSS_CE2):
    cfg = C.GanConfig()
    cfg.g = _spec(g or specs.mixgen_worker(0))
    cfg.d = _spec(d or specs.mnist_discriminator())
    cfg.batch, cfg.batch_real, cfg.epoch = 64, 64, 1
    cfg.loss, cfg.weighting = loss, C.WEIGHT_MIX_SINGLE
    cfg.n_workers, cfg.rank, cfg.exchange_layer = max(W, 1), 0, exchange_layer
    cfg.lr_g = cfg.lr_d = 2e-4
    cfg.beta1, cfg.beta2, cfg.adam_eps = 0.5, 0.999, 1e-8
    cfg.bn_eps, cfg.bn_momentum, cfg.slope = 0.8, 0.1, 0.2
    cfg.seed, cfg.gemm_dtype, cfg.loss_scale = 1, gemm_dtype, loss_scale
    cfg.colocated, cfg.colocated_heads = W, heads
    return cfg


def _ws(cfg):
    return C.lib.cgl_gan_workspace_bytes(ctypes.byref(cfg))


def _al(n):
    return (n + 63) // 64 * 64


def _tensors(cfg):
    out, i = [], 0
    while True:
        off, rows, cols, layer, kind = (ctypes.c_int64(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(),
                                        ctypes.c_int())
        if C.lib.cgl_gan_param_tensor(ctypes.byref(cfg), C.MODEL_G, i, ctypes.byref(off), ctypes.byref(rows),
                                      ctypes.byref(cols), ctypes.byref(layer), ctypes.byref(kind)) != 0:
            return out
        out.append((off.value, rows.value, cols.value, layer.value, kind.value))
        i += 1


@pytest.mark.parametrize("W", [2, 3, C.MAX_COLOCATED])
def test_counts_and_layout(W):
    cfg = _cfg(W)
    m = specs.mixgen_worker(0)
    assert _ws(cfg) > 0
    sizes = []                       # (layer, floats) of every tensor of the trunk + one head, 64-float aligned
    for l in range(m.n_layers):
        fi, fo = m.dims[l], m.dims[l + 1]
        sizes += [(l, _al(fo * fi)), (l, _al(fo))] + ([(l, _al(fo))] * 2 if m.bn[l] else [])
    trunk = sum(n for l, n in sizes if l < XL)
    head = sum(n for l, n in sizes if l >= XL)
    assert C.lib.cgl_gan_param_count(ctypes.byref(cfg), C.MODEL_G) == trunk + W * head
    run_trunk = sum(2 * _al(m.dims[l + 1]) for l in m.bn_layers() if l < XL)
    run_head = sum(2 * _al(m.dims[l + 1]) for l in m.bn_layers() if l >= XL)
    assert C.lib.cgl_gan_running_count(ctypes.byref(cfg)) == run_trunk + W * run_head > 0
    # D's count does not change with the field
    assert C.lib.cgl_gan_param_count(ctypes.byref(cfg), C.MODEL_D) == \
        C.lib.cgl_gan_param_count(ctypes.byref(_cfg(W, heads=0, exchange_layer=-1)), C.MODEL_D)
    # the tensor walk: the trunk, then head 0 .. W - 1 at a constant stride, each tensor 64-float aligned
    ts = _tensors(cfg)
    nt = sum(1 for l, _ in sizes if l < XL)
    nh = len(sizes) - nt
    assert len(ts) == nt + W * nh
    one = _tensors(_cfg(0, heads=0))          # the one-worker Mix-G context: trunk + one head
    assert ts[:nt + nh] == one
    assert [t[3] for t in ts[:nt]] == [l for l, _ in sizes if l < XL]
    assert ts[nt][0] == trunk
    for h in range(W):
        for j in range(nh):
            off, rows, cols, layer, kind = ts[nt + h * nh + j]
            o0, r0, c0, l0, k0 = ts[nt + j]
            assert off == o0 + h * head and off % 64 == 0
            assert (rows, cols, layer, kind) == (r0, c0, l0, k0) and layer >= XL
    last = ts[-1]
    assert last[0] + _al(last[1] * last[2]) == trunk + W * head


def test_workspace_grows_with_the_heads():
    assert _ws(_cfg(4)) > _ws(_cfg(2)) > _ws(_cfg(2, heads=0, exchange_layer=-1))


def test_ring_group_shape():
    """CGLGAN/2DMG: no BatchNorm, a 32-wide exchange tensor, a 2-wide output."""
    cfg = _cfg(2, exchange_layer=specs.RING_HEAD_LAYER, g=specs.ring_generator(0), d=specs.ring_discriminator(),
               loss=C.LOSS_BCE)
    assert _ws(cfg) > 0
    assert C.lib.cgl_gan_param_count(ctypes.byref(cfg), C.MODEL_G) == _al(32 * 100) + _al(32) + 2 * (_al(2 * 32) + 64)
    assert C.lib.cgl_gan_running_count(ctypes.byref(cfg)) == 0


@pytest.mark.parametrize("cfg", [
    _cfg(0),                                                # the field without co-location
    _cfg(1),
    _cfg(3, exchange_layer=-1),                             # no trunk / head split
    _cfg(3, loss_scale=65536.0, gemm_dtype=C.DTYPE_BF16),   # loss scaling
    _cfg(3, heads=2),                                       # the field is 0 / 1
    _cfg(3, heads=0),                                       # field off: the split stays refused
    _cfg(3, heads=0, exchange_layer=2),
], ids=["colocated_0", "colocated_1", "exchange_layer_-1", "loss_scale", "field_2", "field_off", "field_off_layer_2"])
def test_workspace_refuses(cfg):
    assert _ws(cfg) == -1      # CGL_E_ARG


def test_loss_scale_config_is_valid_without_the_heads():
    """The refused loss-scale configuration is refused for the co-location, not for itself."""
    assert _ws(_cfg(0, heads=0, loss_scale=65536.0, gemm_dtype=C.DTYPE_BF16)) > 0


def test_field_off_changes_nothing():
    """With the field 0 a co-located configuration sizes and lays out as a config that never had it."""
    a = _cfg(3, heads=0, exchange_layer=-1, g=specs.mnist_generator())
    assert _ws(a) > 0
    assert _tensors(a) == _tensors(_cfg(0, heads=0, exchange_layer=-1, g=specs.mnist_generator()))


def test_group_spec_keys_are_the_modules():
    torch = pytest.importorskip("torch")  # noqa: F841
    from cglgan import cglgan_2dmg
    from cglgan.model import MixGenerator
    g = specs.mixgen_group(3)
    net = MixGenerator((1, 28, 28), 3)
    assert g.state_keys() == list(net.state_dict().keys())
    assert g.tensor_keys() == [k for k, _ in net.named_parameters()]
    buf = [p + s for p, _, _ in g.running_prefixes() for s in (".running_mean", ".running_var", ".num_batches_tracked")]
    assert sorted(g.tensor_keys() + buf) == sorted(net.state_dict().keys())
    r = specs.ring_group(2)
    rnet = cglgan_2dmg.Generator((2,), 2)
    assert r.state_keys() == r.tensor_keys() == list(rnet.state_dict().keys())
    assert r.running_prefixes() == []
    # a worker's slice is the lockstep form's spec
    assert g.head_spec(2).tensor_keys() == specs.mixgen_worker(2).tensor_keys()
    assert r.head_spec(1).tensor_keys() == specs.ring_generator(1).tensor_keys()


def test_step_refuses_a_one_head_spec():
    """GanStep(colocated=W, exchange_layer=...) with a one-head spec keeps raising (before any device work)."""
    from cglgan import GanStep
    with pytest.raises(ValueError, match="colocated"):
        GanStep(specs.mixgen_worker(0), specs.mnist_discriminator(), batch=64, colocated=3, exchange_layer=XL,
                weighting="mix_single")
    with pytest.raises(ValueError, match="group generator"):
        GanStep(specs.mixgen_group(3), specs.mnist_discriminator(), batch=64, colocated=2, exchange_layer=XL)
    with pytest.raises(ValueError, match="group generator"):
        GanStep(specs.mixgen_group(3), specs.mnist_discriminator(), batch=64, exchange_layer=XL)
