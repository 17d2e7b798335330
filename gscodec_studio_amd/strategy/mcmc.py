"""``MCMCStrategy`` (counterpart of the reference's ``gsplat/strategy/mcmc.py``)."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any, Dict

import torch
from torch import Tensor

from .base import Params, Strategy, reorder_after_refine
from .ops import inject_noise_to_position, relocate, sample_add


@dataclass
class MCMCStrategy(Strategy):
    """The strategy of `3D Gaussian Splatting as Markov Chain Monte Carlo <https://arxiv.org/abs/2404.09591>`_:

    * every step, perturb the means with noise shaped by each gaussian's covariance and gated by its opacity (one random draw and
      one ``gs_inject_noise`` launch);
    * every ``refine_every`` steps, move the gaussians with an opacity of at most ``min_opacity`` onto live ones, and add 5 % new
      gaussians sampled by opacity, up to ``cap_max``.

    Fields as in the reference: ``cap_max``, ``noise_lr``, ``refine_start_iter``, ``refine_stop_iter``, ``refine_every``,
    ``min_opacity``, ``verbose``.  One more: ``reorder`` -- when true, a refinement that changed the set of gaussians ends with
    ``compression.reorder_splats``.

        strategy = MCMCStrategy()
        strategy.check_sanity(params, optimizers)
        state = strategy.initialize_state()
        for step in range(max_steps):
            colors, alphas, info = rasterization(...)
            loss.backward()
            strategy.step_post_backward(params, optimizers, state, step, info, lr=means_lr)
    """

    cap_max: int = 1_000_000
    noise_lr: float = 5e5
    refine_start_iter: int = 500
    refine_stop_iter: int = 25_000
    refine_every: int = 100
    min_opacity: float = 0.005
    verbose: bool = False
    reorder: bool = False

    def initialize_state(self) -> Dict[str, Any]:
        """``binoms [51, 51]``: the binomial coefficients of the relocation formula (moved to the parameters' device on the first step)."""
        n_max = 51
        binoms = torch.zeros((n_max, n_max))
        for n in range(n_max):
            for k in range(n + 1):
                binoms[n, k] = math.comb(n, k)
        return {"binoms": binoms}

    def check_sanity(self, params: Params, optimizers: Dict[str, torch.optim.Optimizer]) -> None:
        super().check_sanity(params, optimizers)
        for key in ["means", "scales", "quats", "opacities"]:
            assert key in params, f"{key} is required in params but missing."

    def step_post_backward(self, params: Params, optimizers: Dict[str, torch.optim.Optimizer], state: Dict[str, Any], step: int,
                           info: Dict[str, Any], lr: float) -> None:
        """``lr``: the current learning rate of ``means``."""
        state["binoms"] = state["binoms"].to(params["means"].device)
        binoms = state["binoms"]

        if step < self.refine_stop_iter and step > self.refine_start_iter and step % self.refine_every == 0:
            n_relocated = self._relocate_gs(params, optimizers, binoms)
            if self.verbose:
                print(f"Step {step}: Relocated {n_relocated} GSs.")
            n_new = self._add_new_gs(params, optimizers, binoms)
            if self.verbose:
                print(f"Step {step}: Added {n_new} GSs. Now having {len(params['means'])} GSs.")
            if self.reorder and n_relocated + n_new > 0:
                reorder_after_refine(params, optimizers, state)
            torch.cuda.empty_cache()

        inject_noise_to_position(params=params, optimizers=optimizers, state={}, scaler=lr * self.noise_lr)

    @torch.no_grad()
    def _relocate_gs(self, params: Params, optimizers: Dict[str, torch.optim.Optimizer], binoms: Tensor) -> int:
        dead_mask = torch.sigmoid(params["opacities"].flatten()) <= self.min_opacity
        n_gs = int(dead_mask.sum().item())
        if n_gs > 0:
            relocate(params=params, optimizers=optimizers, state={}, mask=dead_mask, binoms=binoms, min_opacity=self.min_opacity)
        return n_gs

    @torch.no_grad()
    def _add_new_gs(self, params: Params, optimizers: Dict[str, torch.optim.Optimizer], binoms: Tensor) -> int:
        current = len(params["means"])
        n_target = min(self.cap_max, int(1.05 * current))
        n_gs = max(0, n_target - current)
        if n_gs > 0:
            sample_add(params=params, optimizers=optimizers, state={}, n=n_gs, binoms=binoms, min_opacity=self.min_opacity)
        return n_gs
