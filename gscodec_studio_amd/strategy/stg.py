"""``STG_Strategy`` and ``Modified_STG_Strategy`` (counterparts of the reference's ``gsplat/strategy/STG_Strategy.py`` and
``modified_stg.py``): the densification of the spacetime (dynamic) trainer, ``examples/simple_trainer_dyngs.py``."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, Tuple

import torch
from torch import Tensor

from .base import Params, Strategy, reorder_after_refine
from .default import DefaultStrategy
from .ops import (_param, _update_param_with_optimizer, duplicate, remove, reset_opa, split, stg_freeze_grads,
                  stg_omega_mask)

SPACETIME_KEYS = ("means", "scales", "quats", "opacities", "trbf_scale", "trbf_center", "motion", "omega")


class _SpacetimeStrategy(Strategy):
    """What the two spacetime strategies share: the state, the sanity check, the statistics, the grow / prune masks, the omega mask
    and the removals.  The dataclass fields live on the two classes (their order is the reference's)."""

    key_for_gradient = "means2d"  # (not a field: what DefaultStrategy._update_state reads)
    _prune_by_scale = False

    def initialize_state(self, scene_scale: float = 1.0) -> Dict[str, Any]:
        """The running state: ``grad2d`` / ``count`` (and ``radii`` when ``refine_scale2d_stop_iter > 0``) are allocated on the
        first step, on the device of the gradients."""
        state = {"grad2d": None, "count": None, "scene_scale": scene_scale}
        if self.refine_scale2d_stop_iter > 0:
            state["radii"] = None
        return state

    def check_sanity(self, params: Params, optimizers: Dict[str, torch.optim.Optimizer]) -> None:
        super().check_sanity(params, optimizers)
        for key in SPACETIME_KEYS:
            assert key in params, f"{key} is required in params but missing."

    def step_pre_backward(self, params: Params, optimizers: Dict[str, torch.optim.Optimizer], state: Dict[str, Any], step: int,
                          info: Dict[str, Any]) -> None:
        assert "means2d" in info, "The 2D means of the Gaussians is required but missing."
        info["means2d"].retain_grad()

    def _update_state(self, params: Params, state: Dict[str, Any], info: Dict[str, Any], packed: bool = False) -> None:
        """``DefaultStrategy._update_state``: one ``gs_densify_stats`` launch over ``info["means2d"].grad`` (``.absgrad``)."""
        DefaultStrategy._update_state(self, params, state, info, packed=packed)

    def _zero_stats(self, state: Dict[str, Any]) -> None:
        state["grad2d"].zero_()
        state["count"].zero_()
        if self.refine_scale2d_stop_iter > 0:
            state["radii"].zero_()

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
        if self._prune_by_scale and step > self.reset_every:
            is_too_big = torch.exp(params["scales"]).max(dim=-1).values > self.prune_scale3d * state["scene_scale"]
            if step < self.refine_scale2d_stop_iter:
                is_too_big |= state["radii"] > self.prune_scale2d
            is_prune = is_prune | is_too_big
        n_prune = int(is_prune.sum().item())
        if n_prune > 0:
            remove(params=params, optimizers=optimizers, state=state, mask=is_prune)
        return n_prune

    @torch.no_grad()
    def _zero_omegabymotion(self, params: Params, optimizers: Dict[str, torch.optim.Optimizer], threhold=0.15) -> Tensor:
        """The omega mask (bool ``[N, 1]``: true where omega stays trainable) -- first-order motion ``sum|motion[:, 0:3]| > 0.3``,
        largest scale in (0.2, 0.6), opacity above 0.7 -- in one ``gs_stg_omega_mask`` launch, and ``params["omega"]`` replaced by
        ``mask * omega`` with its optimizer state carried unchanged.  ``threhold`` is unused, as in the reference."""
        mask, omega_new = stg_omega_mask(params["motion"], params["scales"], params["opacities"], params["omega"])

        def param_fn(name: str, p: Tensor) -> Tensor:
            if name != "omega":
                raise ValueError(f"Unexpected parameter name: {name}")
            return _param(omega_new, p)

        _update_param_with_optimizer(param_fn, lambda key, v: v, params, optimizers, names=["omega"])
        return mask

    @torch.no_grad()
    def removeminmax(self, params: Params, optimizers: Dict[str, torch.optim.Optimizer], state: Dict[str, Any], maxbounds,
                     minbounds) -> None:
        """Drop the gaussians whose mean lies outside the box ``minbounds .. maxbounds`` (three tensors or floats each)."""
        maxx, maxy, maxz = (float(v) for v in maxbounds)
        minx, miny, minz = (float(v) for v in minbounds)
        xyz = params["means"]
        mask = ((xyz[:, 0] > maxx) | (xyz[:, 1] > maxy) | (xyz[:, 2] > maxz)
                | (xyz[:, 0] < minx) | (xyz[:, 1] < miny) | (xyz[:, 2] < minz))
        remove(params=params, optimizers=optimizers, state=state, mask=mask)


@dataclass
class STG_Strategy(_SpacetimeStrategy):
    """The densification of `Spacetime Gaussian Feature Splatting <https://arxiv.org/abs/2312.16812>`_ as the reference's dynamic
    trainer runs it (its ``densify = 1`` schedule), hard-coded step numbers included:

    * every step before ``refine_stop_iter``, accumulate the image-plane gradient norms (one ``gs_densify_stats`` launch);
    * every ``refine_every`` steps after ``refine_start_iter``: while ``flag < desicnt``, grow (duplicate / split), zero the
      statistics and count the refinement in ``flag``; after that, prune by opacity only (never by scale) while ``step < 7000``;
    * every ``reset_every`` steps, clamp the opacities to ``2 * prune_opa``;
    * at step 8001 build the omega mask (``_zero_omegabymotion``, one ``gs_stg_omega_mask`` launch: omega is zeroed outside it), and
      on every later step freeze ``omega.grad`` outside the mask and ``quats.grad`` inside it (one ``gs_stg_freeze_grads`` launch, in
      place, no allocation, no host synchronisation);
    * from ``refine_stop_iter`` on: freeze, remove the gaussians with ``z < 4.5`` at ``step % 1000 == 500`` and those outside
      ``minbounds .. maxbounds`` at step 10000, each followed by a rebuilt mask.

    ``step_post_backward`` takes ``flag``, ``desicnt``, ``maxbounds``, ``minbounds`` and returns the (possibly incremented) ``flag``.
    ``omegamask`` (bool ``[N, 1]``) and ``rotationmask`` (its negation) appear on the instance once built, as in the reference.

    Reproduced, not repaired: the step numbers 7000 / 8001 / 10000 and the ``z < 4.5`` cut do not follow the fields; the freeze masks
    are the ones the reference's own comments doubt; growing after step 8001 leaves a mask of the old length behind, which the next
    freeze refuses.  The reference's screen-size term of the prune reads a variable it never assigns; here the prune is by opacity
    alone whatever ``refine_scale2d_stop_iter`` says.

    One more field than the reference: ``reorder`` -- when true, a refinement or removal that changed the set ends with
    ``compression.reorder_splats``; the omega mask is rebuilt after the permutation.

        strategy = STG_Strategy()
        strategy.check_sanity(params, optimizers)
        state = strategy.initialize_state(scene_scale=1.0)
        flag = 0
        for step in range(max_steps):
            colors, alphas, info = render_dynamic(params, t, ...)
            strategy.step_pre_backward(params, optimizers, state, step, info)
            loss.backward()
            flag = strategy.step_post_backward(params, optimizers, state, step, info, flag, desicnt, maxbounds, minbounds)
    """

    prune_opa: float = 0.005
    grow_grad2d: float = 0.0002
    grow_scale3d: float = 0.01
    grow_scale2d: float = 0.05
    prune_scale3d: float = 0.1
    prune_scale2d: float = 0.15
    refine_scale2d_stop_iter: int = 0
    refine_start_iter: int = 500
    refine_stop_iter: int = 9_000
    reset_every: int = 3000
    refine_every: int = 100
    pause_refine_after_reset: int = 0
    absgrad: bool = False
    revised_opacity: bool = False
    verbose: bool = False
    reorder: bool = False

    def _freeze(self, params: Params) -> None:
        mask = self.omegamask
        if getattr(self, "_rotationmask_of", None) is not mask:  # once per mask, not per step
            self.rotationmask = torch.logical_not(mask)
            self._rotationmask_of = mask
        stg_freeze_grads(mask, params["omega"].grad, params["quats"].grad)

    def _after_removal(self, params: Params, optimizers: Dict[str, torch.optim.Optimizer], state: Dict[str, Any], n_before: int) -> None:
        if self.reorder and len(params["means"]) != n_before:
            reorder_after_refine(params, optimizers, state)
        self.omegamask = self._zero_omegabymotion(params, optimizers)

    def step_post_backward(self, params: Params, optimizers: Dict[str, torch.optim.Optimizer], state: Dict[str, Any], step: int,
                           info: Dict[str, Any], flag: int, desicnt: int, maxbounds, minbounds, packed: bool = False) -> int:
        if step >= self.refine_stop_iter:
            self._freeze(params)
            if step % 1000 == 500:
                n = len(params["means"])
                remove(params=params, optimizers=optimizers, state=state, mask=params["means"][:, 2] < 4.5)
                self._after_removal(params, optimizers, state, n)
                torch.cuda.empty_cache()
            if step == 10000:
                n = len(params["means"])
                self.removeminmax(params=params, optimizers=optimizers, state=state, maxbounds=maxbounds, minbounds=minbounds)
                self._after_removal(params, optimizers, state, n)
            return flag

        self._update_state(params, state, info, packed=packed)

        if step == 8001:
            self.omegamask = self._zero_omegabymotion(params, optimizers)
        elif step > 8001:
            self._freeze(params)

        if step > self.refine_start_iter and step % self.refine_every == 0:
            if flag < desicnt:
                n_dupli, n_split = self._grow_gs(params, optimizers, state, step)
                if self.verbose:
                    print(f"Step {step}: {n_dupli} GSs duplicated, {n_split} GSs split. Now having {len(params['means'])} GSs.")
                self._zero_stats(state)
                if self.reorder and n_dupli + n_split > 0:
                    reorder_after_refine(params, optimizers, state)
                torch.cuda.empty_cache()
                flag += 1
            elif step < 7000:
                n_prune = self._prune_gs(params, optimizers, state, step)
                if self.verbose:
                    print(f"Step {step}: {n_prune} GSs pruned. Now having {len(params['means'])} GSs.")
                if self.reorder and n_prune > 0:
                    reorder_after_refine(params, optimizers, state)
                torch.cuda.empty_cache()

        if step % self.reset_every == 0:
            reset_opa(params=params, optimizers=optimizers, state=state, value=self.prune_opa * 2.0)
        return flag


@dataclass
class Modified_STG_Strategy(_SpacetimeStrategy):
    """The reference's modified spacetime strategy: ``DefaultStrategy``'s refinement on the spacetime parameter set.  Every
    ``refine_every`` steps after ``refine_start_iter`` it grows AND prunes (``pause_refine_after_reset`` holds back the prune only;
    after the first reset the prune is also by ``prune_scale3d``), then zeroes the statistics; every ``reset_every`` steps it resets
    the opacities.  It never builds or applies an omega mask in ``step_post_backward`` (``_zero_omegabymotion`` and ``removeminmax``
    exist, as in the reference).  ``step_post_backward`` has ``STG_Strategy``'s signature and returns ``True`` from
    ``refine_stop_iter`` on, ``flag`` unchanged before.

    ``temp_vis_mask`` -- one deliberate difference.  The reference's ``step_pre_backward`` replaces ``info["means2d"]`` by a fresh
    zero tensor of N rows; that tensor has no gradient and its own ``_update_state`` then fails on ``.grad.clone()``.  Here
    ``info["t_vis_mask"]`` is required as there, ``info["means2d"]`` is KEPT when it already has N rows
    (``render_dynamic(temp_vis_mask=True)`` returns full-size rows with ``radii = 0`` for the culled gaussians), and a compacted
    ``means2d`` raises ``ValueError``.

    ``reorder`` as on the other strategies."""

    prune_opa: float = 0.005
    grow_grad2d: float = 0.0002
    grow_scale3d: float = 0.01
    grow_scale2d: float = 0.05
    prune_scale3d: float = 0.1
    prune_scale2d: float = 0.15
    refine_scale2d_stop_iter: int = 0
    refine_start_iter: int = 500
    refine_stop_iter: int = 9_000
    reset_every: int = 3000
    refine_every: int = 100
    pause_refine_after_reset: int = 0
    absgrad: bool = False
    revised_opacity: bool = False
    verbose: bool = False
    temp_vis_mask: bool = False
    reorder: bool = False

    _prune_by_scale = True

    def step_pre_backward(self, params: Params, optimizers: Dict[str, torch.optim.Optimizer], state: Dict[str, Any], step: int,
                          info: Dict[str, Any]) -> None:
        super().step_pre_backward(params, optimizers, state, step, info)
        if self.temp_vis_mask:
            assert "t_vis_mask" in info, "The temporal visible mask of the Gaussians is required but missing."
            n_gaussian = len(list(params.values())[0])
            rows = info["means2d"].shape[-2] if info["means2d"].dim() >= 2 else -1
            if rows != n_gaussian:
                raise ValueError(f"temp_vis_mask: info['means2d'] has {rows} rows for {n_gaussian} gaussians.  It must be full-size "
                                 "(render_dynamic(temp_vis_mask=True) returns it so, with radii = 0 for the culled gaussians): a "
                                 "compacted means2d cannot be replaced by zeros, the replacement would have no gradient.")

    def step_post_backward(self, params: Params, optimizers: Dict[str, torch.optim.Optimizer], state: Dict[str, Any], step: int,
                           info: Dict[str, Any], flag: int, desicnt: int, maxbounds, minbounds, packed: bool = False):
        if step >= self.refine_stop_iter:
            return True
        self._update_state(params, state, info, packed=packed)

        if step > self.refine_start_iter and step % self.refine_every == 0:
            n_dupli, n_split = self._grow_gs(params, optimizers, state, step)
            if self.verbose:
                print(f"Step {step}: {n_dupli} GSs duplicated, {n_split} GSs split. Now having {len(params['means'])} GSs.")
            n_prune = 0
            if step % self.reset_every >= self.pause_refine_after_reset:
                n_prune = self._prune_gs(params, optimizers, state, step)
                if self.verbose:
                    print(f"Step {step}: {n_prune} GSs pruned. Now having {len(params['means'])} GSs.")
            self._zero_stats(state)
            if self.reorder and n_dupli + n_split + n_prune > 0:
                reorder_after_refine(params, optimizers, state)
            torch.cuda.empty_cache()

        if step % self.reset_every == 0:
            reset_opa(params=params, optimizers=optimizers, state=state, value=self.prune_opa * 2.0)
        return flag
