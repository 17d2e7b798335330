"""``DefaultStrategy`` (counterpart of the reference's ``gsplat/strategy/default.py``): the densification of the 3DGS paper."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, Tuple

import torch
from typing_extensions import Literal

from .base import Params, Strategy, reorder_after_refine
from .ops import densify_stats, duplicate, remove, reset_opa, split


@dataclass
class DefaultStrategy(Strategy):
    """The strategy of `3D Gaussian Splatting for Real-Time Radiance Field Rendering <https://arxiv.org/abs/2308.04079>`_:

    * every step, accumulate each visible gaussian's image-plane gradient norm (one ``gs_densify_stats`` launch, no host
      synchronisation);
    * every ``refine_every`` steps, duplicate the gaussians with a high average gradient and a small scale, split those with a
      large scale, and prune those with a low opacity (or, after the first reset, a too large scale);
    * every ``reset_every`` steps, clamp the opacities to ``2 * prune_opa``.

    With ``absgrad=True`` the absolute gradients of `AbsGS <https://arxiv.org/abs/2404.10484>`_ are accumulated
    (``rasterization(..., absgrad=True)``; ``grow_grad2d`` then wants a higher value such as 0.0008).

    Fields as in the reference: ``prune_opa``, ``grow_grad2d``, ``grow_scale3d`` / ``prune_scale3d`` (relative to the scene scale),
    ``grow_scale2d`` / ``prune_scale2d`` (relative to the image, used until ``refine_scale2d_stop_iter``; 0 disables them),
    ``refine_start_iter``, ``refine_stop_iter``, ``reset_every``, ``refine_every``, ``pause_refine_after_reset``, ``absgrad``,
    ``revised_opacity`` (arXiv:2404.06109), ``verbose``, ``key_for_gradient`` (the key of ``info`` whose gradient is accumulated).
    One more: ``reorder`` -- when true, a refinement that changed the set of gaussians ends with
    ``compression.reorder_splats`` (parameters, optimizer state and running statistics in Morton order of the means).

        strategy = DefaultStrategy()
        strategy.check_sanity(params, optimizers)
        state = strategy.initialize_state(scene_scale=1.0)
        for step in range(max_steps):
            colors, alphas, info = rasterization(...)
            strategy.step_pre_backward(params, optimizers, state, step, info)
            loss.backward()
            strategy.step_post_backward(params, optimizers, state, step, info)
    """

    prune_opa: float = 0.005
    grow_grad2d: float = 0.0002
    grow_scale3d: float = 0.01
    grow_scale2d: float = 0.05
    prune_scale3d: float = 0.1
    prune_scale2d: float = 0.15
    refine_scale2d_stop_iter: int = 0
    refine_start_iter: int = 500
    refine_stop_iter: int = 15_000
    reset_every: int = 3000
    refine_every: int = 100
    pause_refine_after_reset: int = 0
    absgrad: bool = False
    revised_opacity: bool = False
    verbose: bool = False
    key_for_gradient: Literal["means2d", "gradient_2dgs"] = "means2d"
    reorder: bool = False

    def initialize_state(self, scene_scale: float = 1.0) -> Dict[str, Any]:
        """The running state: ``grad2d`` / ``count`` (and ``radii`` when ``refine_scale2d_stop_iter > 0``) are allocated on the
        first step, on the device of the gradients."""
        state = {"grad2d": None, "count": None, "scene_scale": scene_scale}
        if self.refine_scale2d_stop_iter > 0:
            state["radii"] = None
        return state

    def check_sanity(self, params: Params, optimizers: Dict[str, torch.optim.Optimizer]) -> None:
        super().check_sanity(params, optimizers)
        for key in ["means", "scales", "quats", "opacities"]:
            assert key in params, f"{key} is required in params but missing."

    def step_pre_backward(self, params: Params, optimizers: Dict[str, torch.optim.Optimizer], state: Dict[str, Any], step: int,
                          info: Dict[str, Any]) -> None:
        assert self.key_for_gradient in info, "The 2D means of the Gaussians is required but missing."
        info[self.key_for_gradient].retain_grad()

    def step_post_backward(self, params: Params, optimizers: Dict[str, torch.optim.Optimizer], state: Dict[str, Any], step: int,
                           info: Dict[str, Any], packed: bool = False) -> None:
        if step >= self.refine_stop_iter:
            return
        self._update_state(params, state, info, packed=packed)

        if (step > self.refine_start_iter and step % self.refine_every == 0
                and step % self.reset_every >= self.pause_refine_after_reset):
            n_dupli, n_split = self._grow_gs(params, optimizers, state, step)
            if self.verbose:
                print(f"Step {step}: {n_dupli} GSs duplicated, {n_split} GSs split. Now having {len(params['means'])} GSs.")
            n_prune = self._prune_gs(params, optimizers, state, step)
            if self.verbose:
                print(f"Step {step}: {n_prune} GSs pruned. Now having {len(params['means'])} GSs.")
            state["grad2d"].zero_()
            state["count"].zero_()
            if self.refine_scale2d_stop_iter > 0:
                state["radii"].zero_()
            if self.reorder and n_dupli + n_split + n_prune > 0:
                reorder_after_refine(params, optimizers, state)
            torch.cuda.empty_cache()

        if step % self.reset_every == 0:
            reset_opa(params=params, optimizers=optimizers, state=state, value=self.prune_opa * 2.0)

    def _update_state(self, params: Params, state: Dict[str, Any], info: Dict[str, Any], packed: bool = False) -> None:
        """One ``gs_densify_stats`` launch over ``info[key_for_gradient].grad`` (``.absgrad``), read in place."""
        for key in ["width", "height", "n_cameras", "radii", "gaussian_ids", self.key_for_gradient]:
            assert key in info, f"{key} is required but missing."
        grads = info[self.key_for_gradient].absgrad if self.absgrad else info[self.key_for_gradient].grad
        n_gaussian = len(list(params.values())[0])
        for key in ("grad2d", "count") + (("radii",) if self.refine_scale2d_stop_iter > 0 else ()):
            if state[key] is None:
                state[key] = torch.zeros(n_gaussian, device=grads.device)
        densify_stats(grads, info["radii"], info["gaussian_ids"] if packed else None, info["width"], info["height"],
                      info["n_cameras"], state["grad2d"], state["count"],
                      state["radii"] if self.refine_scale2d_stop_iter > 0 else None)

    @torch.no_grad()
    def _grow_gs(self, params: Params, optimizers: Dict[str, torch.optim.Optimizer], state: Dict[str, Any], step: int) -> Tuple[int, int]:
        count = state["count"]
        grads = state["grad2d"] / count.clamp_min(1)
        is_grad_high = grads > self.grow_grad2d
        is_small = torch.exp(params["scales"]).max(dim=-1).values <= self.grow_scale3d * state["scene_scale"]
        is_dupli = is_grad_high & is_small
        n_dupli = int(is_dupli.sum().item())
        is_split = is_grad_high & ~is_small
        if step < self.refine_scale2d_stop_iter:
            is_split |= state["radii"] > self.grow_scale2d
        n_split = int(is_split.sum().item())

        if n_dupli > 0:
            duplicate(params=params, optimizers=optimizers, state=state, mask=is_dupli)
        # the copies appended by the duplication are not split
        is_split = torch.cat([is_split, torch.zeros(n_dupli, dtype=torch.bool, device=grads.device)])
        if n_split > 0:
            split(params=params, optimizers=optimizers, state=state, mask=is_split, revised_opacity=self.revised_opacity)
        return n_dupli, n_split

    @torch.no_grad()
    def _prune_gs(self, params: Params, optimizers: Dict[str, torch.optim.Optimizer], state: Dict[str, Any], step: int) -> int:
        is_prune = torch.sigmoid(params["opacities"].flatten()) < self.prune_opa
        if step > self.reset_every:
            is_too_big = torch.exp(params["scales"]).max(dim=-1).values > self.prune_scale3d * state["scene_scale"]
            # (screen-size pruning: off by default, refine_scale2d_stop_iter = 0, as in the official implementation)
            if step < self.refine_scale2d_stop_iter:
                is_too_big |= state["radii"] > self.prune_scale2d
            is_prune = is_prune | is_too_big
        n_prune = int(is_prune.sum().item())
        if n_prune > 0:
            remove(params=params, optimizers=optimizers, state=state, mask=is_prune)
        return n_prune
