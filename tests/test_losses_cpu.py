"""gscodec_studio_amd.losses without a GPU: the module imports and exports its two functions, every input outside the contract is
refused with a ValueError that names the problem, the SSIM window is the float32 normalised Gaussian, and the loss entry points are
part of the C ABI and refuse null pointers before any launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_module_imports_and_exports():
    from gscodec_studio_amd import losses

    assert set(losses.__all__) == {"fused_ssim", "photometric_loss"}
    assert callable(losses.fused_ssim) and callable(losses.photometric_loss)
    assert "fused_ssim" in losses.__doc__ and "photometric_loss" in losses.__doc__


def _img(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


@pytest.mark.parametrize("args, match", [
    ((_img(1, 3, 16, 16, dtype=torch.float64), _img(1, 3, 16, 16)), "float32"),
    ((_img(1, 3, 16, 16, dtype=torch.float16), _img(1, 3, 16, 16, dtype=torch.float16)), "float32"),
    ((_img(3, 16, 16), _img(3, 16, 16)), "4-D"),
    ((_img(1, 1, 3, 16, 16), _img(1, 1, 3, 16, 16)), "4-D"),
    ((_img(1, 3, 16, 16), _img(1, 3, 16, 17)), "same shape"),
    ((_img(1, 3, 16, 16), _img(1, 3, 16, 16)), "GPU"),
])
def test_fused_ssim_refuses(args, match):
    from gscodec_studio_amd.losses import fused_ssim

    with pytest.raises(ValueError, match=match):
        fused_ssim(*args)


def test_fused_ssim_refuses_padding_size_and_small_valid():
    from gscodec_studio_amd.losses import fused_ssim

    a = _img(1, 3, 16, 16)
    with pytest.raises(ValueError, match="padding"):
        fused_ssim(a, a, padding="reflect")
    big = torch.zeros(1).expand(1, 1, 65536, 32768)  # 2^31 elements, no memory behind them
    with pytest.raises(ValueError, match="2\\^31"):
        fused_ssim(big, big)
    for h, w in ((10, 64), (64, 10), (11, 5)):
        with pytest.raises(ValueError, match="valid"):
            fused_ssim(_img(1, 3, h, w), _img(1, 3, h, w), padding="valid")


def test_photometric_loss_refuses():
    from gscodec_studio_amd.losses import photometric_loss

    a = _img(1, 16, 16, 3)
    with pytest.raises(ValueError, match="float32"):
        photometric_loss(a.double(), a)
    with pytest.raises(ValueError, match="4-D"):
        photometric_loss(a[0], a[0])
    with pytest.raises(ValueError, match="same shape"):
        photometric_loss(a, _img(1, 16, 17, 3))
    with pytest.raises(ValueError, match="padding"):
        photometric_loss(a, a, padding="full")
    with pytest.raises(ValueError, match="valid"):
        photometric_loss(_img(1, 10, 64, 3), _img(1, 10, 64, 3))
    with pytest.raises(ValueError, match="GPU"):
        photometric_loss(a, a)


def test_ssim_window_is_the_float32_normalised_gaussian():
    from gscodec_studio_amd import _wrapper as W

    g = np.exp(-((np.arange(11) - 5.0) ** 2) / 4.5)
    want = (g / g.sum()).astype(np.float32)
    got = np.array(W.ssim_window(), dtype=np.float32)
    assert got.shape == (11,)
    assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist()


def test_ssim_entry_points_are_declared_exported_and_refuse_null_pointers():
    from gscodec_studio_amd import _backend as B
    from gscodec_studio_amd import _wrapper as W

    protos = B.prototypes()
    hdr = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    for name in ("gs_ssim_fwd", "gs_ssim_bwd", "gs_ssim_work_bytes", "gs_ssim_window"):
        assert name in protos and name + "(" in hdr, name
        assert hasattr(B.lib(), name), name
    # the work area grows by the three coefficient maps with train
    assert W.ssim_work_bytes((2, 3, 37, 53), True) - W.ssim_work_bytes((2, 3, 37, 53), False) >= 3 * 4 * 2 * 3 * 37 * 53
    st = (ctypes.c_int64 * 4)(3 * 37 * 53, 37 * 53, 53, 1)
    with pytest.raises(RuntimeError, match="null pointer"):
        B.call("gs_ssim_fwd", None, ctypes.addressof(st), None, ctypes.addressof(st), 2, 3, 37, 53, 0, 1, 0.2, None, 0, None, None,
               None, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        B.call("gs_ssim_bwd", None, ctypes.addressof(st), None, ctypes.addressof(st), 2, 3, 37, 53, 0, None, 0, None, 1.0, None, 0.0,
               None, ctypes.addressof(st), None)
    # a bad shape is refused before any launch too (fake, never dereferenced, non-null pointers)
    with pytest.raises(RuntimeError, match="valid padding"):
        B.call("gs_ssim_fwd", 64, ctypes.addressof(st), 64, ctypes.addressof(st), 1, 1, 8, 8, 1, 0, 0.2, 256, 1 << 20, 64, None, None,
               None)
    with pytest.raises(RuntimeError, match="2\\^31"):
        B.call("gs_ssim_fwd", 64, ctypes.addressof(st), 64, ctypes.addressof(st), 1, 1, 65536, 32768, 0, 0, 0.2, 256, 1 << 20, 64,
               None, None, None)
