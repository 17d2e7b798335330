"""The interface of a densification strategy (counterpart of the reference's ``gsplat/strategy/base.py``)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, Union

import torch

Params = Union[Dict[str, torch.nn.Parameter], torch.nn.ParameterDict]


@dataclass
class Strategy:
    """Base class: ``check_sanity`` and the two callbacks of the training loop (no-ops here)."""

    def check_sanity(self, params: Params, optimizers: Dict[str, torch.optim.Optimizer]) -> None:
        """The trainable parameters and the optimizers must have the same names, one parameter group per optimizer."""
        trainable = {name for name, p in params.items() if p.requires_grad}
        assert trainable == set(optimizers.keys()), ("trainable parameters and optimizers must have the same keys, "
                                                     f"but got {trainable} and {optimizers.keys()}")
        for opt in optimizers.values():
            assert len(opt.param_groups) == 1, ("Each optimizer must have exactly one param_group, that corresponds to each "
                                                f"parameter, but got {len(opt.param_groups)}")

    def step_pre_backward(self, *args, **kwargs) -> None:
        """Called before ``loss.backward()``."""

    def step_post_backward(self, *args, **kwargs) -> None:
        """Called after ``loss.backward()``."""


def reorder_after_refine(params: Params, optimizers: Dict[str, torch.optim.Optimizer], state: Dict[str, Any]) -> None:
    """The ``reorder=True`` option of both strategies: ``compression.reorder_splats`` (Morton order of the means) over the
    parameters, their optimizer state and the per-gaussian tensors of ``state``; other entries of ``state`` (scalars, the MCMC
    binomial table) are not handed over."""
    from ..compression import reorder_splats

    n = int(params["means"].shape[0])
    per_gaussian = {k: v for k, v in state.items() if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == n and k != "binoms"}
    reorder_splats(params, optimizers, state=per_gaussian)
    state.update(per_gaussian)
