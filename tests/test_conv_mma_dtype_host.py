"""cgl_conv_set_mma_dtype / cgl_conv_get_mma_dtype (the MFMA convolution kernels' operand type) on the host: the
thread-local mode, its argument and state checks and the ``conv_ops.mma_dtype`` context manager.  None of these calls
touches a device, so the file runs on CPU.
"""
import os
import re

import pytest

from cglgan import _lib as C
from cglgan import conv_ops as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_STATE = -1, -2


@pytest.fixture(autouse=True)
def _f32_mode():
    """Every test starts and must end in the default mode."""
    assert C.lib.cgl_conv_get_mma_dtype() == C.DTYPE_F32
    yield
    assert C.lib.cgl_conv_get_mma_dtype() == C.DTYPE_F32


def test_default_is_f32():
    assert C.lib.cgl_conv_get_mma_dtype() == C.DTYPE_F32 == 0
    assert O.get_mma_dtype() == C.DTYPE_F32


def test_set_get_roundtrip():
    lib = C.lib
    assert lib.cgl_conv_set_mma_dtype(C.DTYPE_BF16) == 0
    try:
        assert lib.cgl_conv_get_mma_dtype() == C.DTYPE_BF16
        assert O.get_mma_dtype() == C.DTYPE_BF16
    finally:
        assert lib.cgl_conv_set_mma_dtype(C.DTYPE_F32) == 0
    assert lib.cgl_conv_get_mma_dtype() == C.DTYPE_F32


@pytest.mark.parametrize("mode", [C.DTYPE_F32, C.DTYPE_BF16])
@pytest.mark.parametrize("bad", [C.DTYPE_F16, 7, -1])
def test_bad_dtype_is_refused_and_changes_nothing(mode, bad):
    lib = C.lib
    assert lib.cgl_conv_set_mma_dtype(mode) == 0
    try:
        assert lib.cgl_conv_set_mma_dtype(bad) == E_ARG
        assert lib.cgl_conv_get_mma_dtype() == mode
    finally:
        assert lib.cgl_conv_set_mma_dtype(C.DTYPE_F32) == 0


def test_refused_inside_a_launch_batch():
    lib = C.lib
    assert lib.cgl_conv_batch_begin(None) == 0
    try:
        assert lib.cgl_conv_set_mma_dtype(C.DTYPE_BF16) == E_STATE
        assert lib.cgl_conv_set_mma_dtype(C.DTYPE_F32) == E_STATE
        assert lib.cgl_conv_get_mma_dtype() == C.DTYPE_F32
    finally:
        assert lib.cgl_conv_batch_end(None) == 0      # (an empty batch launches nothing)
    assert lib.cgl_conv_set_mma_dtype(C.DTYPE_BF16) == 0
    assert lib.cgl_conv_set_mma_dtype(C.DTYPE_F32) == 0


def test_refused_inside_a_wgrad_deferral():
    lib = C.lib
    assert lib.cgl_conv_wgrad_defer_begin() == 0
    try:
        assert lib.cgl_conv_set_mma_dtype(C.DTYPE_BF16) == E_STATE
        assert lib.cgl_conv_get_mma_dtype() == C.DTYPE_F32
    finally:
        assert lib.cgl_conv_wgrad_defer_end(None) == 0     # (nothing recorded: launches nothing)
    assert lib.cgl_conv_set_mma_dtype(C.DTYPE_BF16) == 0
    assert lib.cgl_conv_set_mma_dtype(C.DTYPE_F32) == 0


def test_context_manager_sets_and_restores():
    with O.mma_dtype("bf16"):
        assert O.get_mma_dtype() == C.DTYPE_BF16
        with O.mma_dtype("f32"):
            assert O.get_mma_dtype() == C.DTYPE_F32
        assert O.get_mma_dtype() == C.DTYPE_BF16
        with O.mma_dtype(C.DTYPE_BF16):      # the enum is accepted as well
            assert O.get_mma_dtype() == C.DTYPE_BF16
    assert O.get_mma_dtype() == C.DTYPE_F32


def test_context_manager_restores_after_an_exception():
    class Boom(Exception):
        pass

    with pytest.raises(Boom):
        with O.mma_dtype("bf16"):
            assert O.get_mma_dtype() == C.DTYPE_BF16
            raise Boom()
    assert O.get_mma_dtype() == C.DTYPE_F32


def test_context_manager_refuses_f16_and_unknown_names():
    with pytest.raises(ValueError, match="loss scaling"):
        with O.mma_dtype("f16"):
            pass
    with pytest.raises(ValueError):
        with O.mma_dtype("fp8"):
            pass
    with pytest.raises(RuntimeError):             # the enum's f16: refused by the library (CGL_E_ARG)
        with O.mma_dtype(C.DTYPE_F16):
            pass
    assert O.get_mma_dtype() == C.DTYPE_F32


def test_mode_is_thread_local():
    import threading
    seen = {}

    def other():
        seen["start"] = C.lib.cgl_conv_get_mma_dtype()
        seen["rc"] = C.lib.cgl_conv_set_mma_dtype(C.DTYPE_F32)

    with O.mma_dtype("bf16"):
        t = threading.Thread(target=other)
        t.start()
        t.join()
        assert O.get_mma_dtype() == C.DTYPE_BF16
    assert seen == {"start": C.DTYPE_F32, "rc": 0}


def test_header_and_exports_in_step():
    src = open(os.path.join(ROOT, "include", "cglgan.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("cgl_conv_set_mma_dtype", "cgl_conv_get_mma_dtype"):
        assert re.search(rf"\bint {name}\s*\(", src), name
        assert name in C.EXPORTS
        assert hasattr(C.lib, name)
