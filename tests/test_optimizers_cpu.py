"""gscodec_studio_amd.optimizers without a GPU: the module imports, unsupported Adam settings are refused at construction,
the host-side descriptor scalars equal torch's Adam arithmetic, and the optimizer entry points are part of the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_module_imports_and_exports():
    import gscodec_studio_amd
    from gscodec_studio_amd import optimizers
    from gscodec_studio_amd._c_adapter import _C

    for name in ("Adam", "SelectiveAdam", "step_all", "visibility_mask"):
        assert callable(getattr(optimizers, name)), name
    assert issubclass(optimizers.Adam, torch.optim.Adam) and issubclass(optimizers.SelectiveAdam, torch.optim.Adam)
    assert callable(gscodec_studio_amd.selective_adam_update) and callable(_C.selective_adam_update)


@pytest.mark.parametrize("kw", [dict(amsgrad=True), dict(weight_decay=1e-4), dict(maximize=True), dict(capturable=True),
                                dict(differentiable=True), dict(fused=True), dict(lr=torch.tensor(1e-3))])
def test_adam_refuses_unsupported_settings(kw):
    from gscodec_studio_amd.optimizers import Adam

    p = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises((ValueError, RuntimeError)):
        Adam([p], **kw)


def test_adam_refuses_unsupported_group_and_accepts_supported():
    from gscodec_studio_amd.optimizers import Adam

    p, q = torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(4))
    opt = Adam([{"params": [p], "lr": 1e-2, "name": "means"}], eps=1e-15, betas=(0.9, 0.999), foreach=True)
    with pytest.raises(ValueError, match="weight_decay"):
        opt.add_param_group({"params": [q], "weight_decay": 0.1})
    # the state dict has torch.optim.Adam's layout: a plain torch Adam loads it
    torch.optim.Adam([torch.nn.Parameter(torch.zeros(4))], lr=1e-2).load_state_dict(opt.state_dict())


def test_step_needs_gpu_tensors_and_names_the_parameter():
    from gscodec_studio_amd.optimizers import Adam, step_all

    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    opt = Adam([{"params": [p], "name": "opacities"}])
    with pytest.raises(RuntimeError, match="opacities"):
        opt.step()
    assert len(opt.state) == 0  # nothing was initialised or advanced
    with pytest.raises(TypeError):
        step_all([torch.optim.SGD([p], lr=0.1)])


def test_dense_descriptor_scalars_equal_torch_formula():
    """step_size = lr / (1 - b1^step), bc2_sqrt = (1 - b2^step)^0.5 in double (torch.optim.adam._single_tensor_adam),
    1 - b1 / 1 - b2 (the lerp / addcmul weights) -- each rounded once to float in the descriptor."""
    from gscodec_studio_amd import _wrapper as W

    lr, beta1, beta2, eps = 1.6e-4 * 0.7, 0.9, 0.999, 1e-15
    t = torch.zeros(8)
    for step in (1, 2, 1000):
        d = W.adam_desc(W.ADAM_DENSE, t, t, t, t, lr, beta1, beta2, eps, step=float(step))
        f32 = lambda x: float(np.float32(x))  # noqa: E731
        assert d.step_size == f32(lr / (1 - beta1 ** step)), step
        assert d.bias_correction2_sqrt == f32((1 - beta2 ** step) ** 0.5), step
        assert d.one_minus_beta1 == f32(1 - beta1) and d.one_minus_beta2 == f32(1 - beta2)
        assert d.beta2 == f32(beta2) and d.eps == f32(eps) and d.n == 8 and d.mode == W.ADAM_DENSE
    # the selective descriptor carries the reference's float arguments and the row split
    vis = torch.ones(4, dtype=torch.bool)
    d = W.adam_desc(W.ADAM_SELECTIVE, t, t, t, t, 1e-3, 0.9, 0.999, 1e-15, visibility=vis, rows=4, row_width=2, n=8)
    assert (d.rows, d.row_width, d.n, d.mode) == (4, 2, 8, W.ADAM_SELECTIVE) and d.lr == float(np.float32(1e-3))


def test_adam_multi_is_declared_exported_and_mirrored():
    from gscodec_studio_amd import _backend as B
    from gscodec_studio_amd import _wrapper as W

    protos = B.prototypes()
    for name in ("gs_adam_multi", "gs_adam_multi_max", "gs_adam_desc_layout"):
        assert name in protos, name
        assert hasattr(B.lib(), name), name
    hdr = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    assert int(re.search(r"#define GS_ADAM_MULTI_MAX (\d+)", hdr).group(1)) == int(B.query("gs_adam_multi_max"))
    W.check_adam_desc_layout()
    # a bad descriptor is refused before anything is launched (no device needed to reach the check)
    bad = W._AdamDesc()
    bad.n, bad.mode = 16, 7
    table = (W._AdamDesc * 1)(bad)
    with pytest.raises(RuntimeError, match="null pointer|unknown mode"):
        B.call("gs_adam_multi", 1, ctypes.addressof(table), None)
