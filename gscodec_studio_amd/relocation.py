"""``compute_relocation`` (counterpart of the reference's ``gsplat/relocation.py``) on the ``gs_relocation`` HIP kernel."""
from __future__ import annotations

from typing import Tuple

import torch
from torch import Tensor

from . import _backend as B
from ._wrapper import _device_of, _f32c, _require_gpu, _stream

__all__ = ["compute_relocation"]


def relocation_native(opacities: Tensor, scales: Tensor, ratios: Tensor, binoms: Tensor, n_max: int) -> Tuple[Tensor, Tensor]:
    """The native entry with the reference's positional signature (``compute_relocation_tensor``, csrc/compute_relocation.cu:40-74):
    contiguous float32 ``opacities [N]``, ``scales [N, 3]``, ``binoms [n_max, n_max]`` and int32 ``ratios [N]`` in ``[1, n_max]``."""
    _require_gpu(opacities, "compute_relocation")
    for t, what in ((scales, "scales"), (ratios, "ratios"), (binoms, "binoms")):
        _require_gpu(t, f"compute_relocation ({what})")
        if t.device != opacities.device:
            raise RuntimeError(f"compute_relocation: {what} is on {t.device}, opacities on {opacities.device}")
    if ratios.dtype != torch.int32:
        raise RuntimeError(f"compute_relocation: ratios must be int32, got {ratios.dtype}")
    opacities, scales, binoms, ratios = _f32c(opacities), _f32c(scales), _f32c(binoms), ratios.contiguous()
    N = opacities.shape[0]
    if scales.shape != (N, 3) or ratios.shape != (N,) or opacities.dim() != 1:
        raise RuntimeError(f"compute_relocation: opacities {tuple(opacities.shape)}, scales {tuple(scales.shape)}, ratios "
                           f"{tuple(ratios.shape)}: expected [N], [N, 3], [N]")
    if binoms.dim() != 2 or binoms.shape[0] != binoms.shape[1] or binoms.shape[0] != int(n_max):
        raise RuntimeError(f"compute_relocation: binoms is {tuple(binoms.shape)}, expected [{int(n_max)}, {int(n_max)}]")
    new_opacities, new_scales = torch.empty_like(opacities), torch.empty_like(scales)
    with _device_of(opacities):
        B.call("gs_relocation", N, B.ptr(opacities), B.ptr(scales), B.ptr(ratios), B.ptr(binoms), int(n_max), B.ptr(new_opacities),
               B.ptr(new_scales), _stream(opacities))
    return new_opacities, new_scales


def compute_relocation(opacities: Tensor, scales: Tensor, ratios: Tensor, binoms: Tensor) -> Tuple[Tensor, Tensor]:
    """New opacities and scales for gaussians that each stand for ``ratios[i]`` copies of themselves: equation 9 of
    `3D Gaussian Splatting as Markov Chain Monte Carlo <https://arxiv.org/abs/2404.09591>`_.

    ``opacities [N]``, ``scales [N, 3]`` (both activated), ``ratios [N]`` (integer; clamped IN PLACE to ``[1, n_max]``, as the
    reference does), ``binoms [n_max, n_max]`` with ``binoms[n, k] = C(n, k)``.  Returns ``(new_opacities [N], new_scales [N, 3])``
    with ``new_opacity = 1 - (1 - o)^(1/n)`` and ``new_scale = scale * o / sum_{i=1..n} sum_{k<i} binoms[i-1, k] (-1)^k /
    sqrt(k+1) * new_opacity^(k+1)``.  The kernel evaluates both in double and rounds once (the reference's float loop is off by up
    to a few 1e-4 at large n)."""
    N = opacities.shape[0]
    n_max, _ = binoms.shape
    assert scales.shape == (N, 3), scales.shape
    assert ratios.shape == (N,), ratios.shape
    _require_gpu(opacities, "compute_relocation")
    ratios.clamp_(min=1, max=n_max)
    return relocation_native(opacities, scales, ratios.int(), binoms, n_max)
