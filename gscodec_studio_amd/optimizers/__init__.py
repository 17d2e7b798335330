"""Optimizers for the splat parameters (counterpart of the reference's ``gsplat.optimizers``), stepped by one HIP kernel.

* ``SelectiveAdam(params, eps, betas)`` -- the reference's ``gsplat/optimizers/selective_adam.py``: ``step(visibility)`` updates
  only the rows whose visibility is set (the trainers' ``--visible_adam``), same state layout (``step`` stays 0).
* ``Adam`` -- a drop-in ``torch.optim.Adam`` (same constructor, same ``step(closure=None)``, same state: ``step`` a CPU float32
  tensor advanced by one per step, ``exp_avg``, ``exp_avg_sq``), so ``state_dict`` / ``load_state_dict`` work both ways with
  ``torch.optim.Adam`` and LR schedulers keep working.  Settings the kernel does not cover raise ``ValueError``.
* ``step_all(optimizers, visibility=None)`` -- the trainer's ``for opt in optimizers.values(): opt.step(); opt.zero_grad(...)``
  loop as ONE ``gs_adam_multi`` call over every parameter of every optimizer (``Adam``, plain ``torch.optim.Adam`` with
  supported settings, ``SelectiveAdam``).
* ``visibility_mask(meta, n)`` -- the trainer's ``visible_adam`` mask from ``rasterization()``'s meta.
* ``SparseAdam`` -- a drop-in ``torch.optim.SparseAdam`` for the trainers' ``--sparse_grad`` mode, and ``sparsify_grads(params,
  gaussian_ids, coalesced)``, the trainer's loop that builds the COO gradients (``optimizers/sparse.py``).  ``step_all`` takes
  ``SparseAdam`` optimizers next to the dense ones: all their gradients over one index list cost one sort and one
  ``gs_sparse_adam_multi`` launch.

There is no fallback to torch's own Adam: a parameter the kernel cannot step raises.
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Union

import torch
from torch import Tensor

from .. import _wrapper as W

__all__ = ["Adam", "SelectiveAdam", "SparseAdam", "step_all", "sparsify_grads", "visibility_mask"]


def _check_group(group: dict) -> None:
    """Refuse the torch.optim.Adam settings the kernel does not implement."""
    if isinstance(group.get("lr"), Tensor):
        raise ValueError("gscodec_studio_amd.optimizers: a tensor lr is not supported (pass a float)")
    if any(isinstance(b, Tensor) for b in group.get("betas", ())):
        raise ValueError("gscodec_studio_amd.optimizers: tensor betas are not supported (pass floats)")
    if group.get("amsgrad", False):
        raise ValueError("gscodec_studio_amd.optimizers: amsgrad=True is not supported")
    if group.get("weight_decay", 0) != 0:
        raise ValueError("gscodec_studio_amd.optimizers: weight_decay != 0 is not supported")
    for key in ("maximize", "capturable", "differentiable", "fused"):
        if group.get(key, False):
            raise ValueError(f"gscodec_studio_amd.optimizers: {key}=True is not supported")


def _param_name(group: dict, gi: int, pi: int) -> str:
    name = group.get("name")
    return f"{name!r}" if name is not None and len(group["params"]) == 1 else f"param_groups[{gi}]['params'][{pi}]" + (
        f" ({name!r})" if name is not None else "")


def _check_param(p: Tensor, group: dict, gi: int, pi: int) -> None:
    g = p.grad
    what = _param_name(group, gi, pi)
    if g.is_sparse:
        raise RuntimeError(f"gscodec_studio_amd.optimizers: parameter {what} has a sparse gradient (not supported)")
    for t, kind in ((p, "parameter"), (g, "gradient")):
        if not t.is_cuda:
            raise RuntimeError(f"gscodec_studio_amd.optimizers: {kind} of {what} is on {t.device}; the HIP step needs a GPU tensor")
        if t.dtype != torch.float32:
            raise RuntimeError(f"gscodec_studio_amd.optimizers: {kind} of {what} is {t.dtype}; only float32 is supported")
        if not t.is_contiguous():
            raise RuntimeError(f"gscodec_studio_amd.optimizers: {kind} of {what} is not contiguous")
    if g.shape != p.shape or g.device != p.device:
        raise RuntimeError(f"gscodec_studio_amd.optimizers: gradient of {what} does not match the parameter's shape / device")


def _check_state(opt: torch.optim.Optimizer, p: Tensor, what: str) -> None:
    st = opt.state.get(p)
    if not st:
        return
    for k in ("exp_avg", "exp_avg_sq"):
        t = st[k]
        if not (t.shape == p.shape and t.device == p.device and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError(f"gscodec_studio_amd.optimizers: state {k!r} of {what} does not match the parameter "
                               "(contiguous float32, same shape and device)")


def _init_state(opt: torch.optim.Optimizer, p: Tensor) -> dict:
    st = opt.state[p]
    if len(st) == 0:  # torch.optim.Adam's lazy state (non-capturable, non-fused): a CPU float32 step
        st["step"] = torch.tensor(0.0, dtype=torch.float32)
        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
    return st


def _visibility(vis: Tensor, like: Tensor) -> Tensor:
    if vis.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError(f"gscodec_studio_amd.optimizers: visibility must be bool or uint8, got {vis.dtype}")
    if vis.device != like.device:
        raise RuntimeError(f"gscodec_studio_amd.optimizers: visibility is on {vis.device}, the parameters on {like.device}")
    return vis.contiguous()


def _validate(opt: torch.optim.Optimizer, selective: bool, visibility: Optional[Tensor]) -> None:
    """Every check of a step, before anything is mutated."""
    if selective and visibility is None:
        raise ValueError("gscodec_studio_amd.optimizers: SelectiveAdam needs a visibility mask")
    for gi, group in enumerate(opt.param_groups):
        if selective:
            assert len(group["params"]) == 1, "more than one tensor in group"
        else:
            _check_group(group)
        for pi, p in enumerate(group["params"]):
            if p.grad is None:
                continue
            _check_param(p, group, gi, pi)
            _check_state(opt, p, _param_name(group, gi, pi))
            if selective:
                if visibility.dim() > 1 and visibility.numel() != visibility.shape[0]:
                    raise RuntimeError("gscodec_studio_amd.optimizers: visibility must have shape [N]")
                _visibility(visibility, p)


def _collect(opt: torch.optim.Optimizer, selective: bool, visibility: Optional[Tensor], out: List) -> None:
    """Append one descriptor per parameter with a gradient; advances the dense step counters as ``opt.step()`` would."""
    vis = None
    for group in opt.param_groups:
        lr, eps = group["lr"], group["eps"]
        beta1, beta2 = group["betas"]
        for p in group["params"]:
            if p.grad is None:
                continue
            st = _init_state(opt, p)
            if selective:  # gsplat/optimizers/selective_adam.py: N = visibility.numel(), M = numel // N, step never advanced
                if vis is None:
                    vis = _visibility(visibility, p)
                N = vis.numel()
                M = p.numel() // N if N else 0
                if M == 0:
                    continue
                out.append((p, W.adam_desc(W.ADAM_SELECTIVE, p, p.grad, st["exp_avg"], st["exp_avg_sq"], lr, beta1, beta2, eps,
                                           visibility=vis, rows=N, row_width=M, n=N * M), vis))  # (vis: kept alive to the launch)
            else:
                st["step"] += 1
                out.append((p, W.adam_desc(W.ADAM_DENSE, p, p.grad, st["exp_avg"], st["exp_avg_sq"], lr, beta1, beta2, eps,
                                           step=st["step"].item()), None))


def _launch(entries: List) -> None:
    by_dev: Dict[torch.device, List] = {}
    for p, d, _ in entries:
        by_dev.setdefault(p.device, []).append((p, d))
    for items in by_dev.values():
        W.adam_multi([d for _, d in items], items[0][0])


class Adam(torch.optim.Adam):
    """``torch.optim.Adam`` stepped by the HIP kernel (``gs_adam_multi``, one launch per ``step``): the same constructor, state
    layout and step semantics as torch's non-capturable, non-fused Adam.  ``amsgrad``, ``weight_decay != 0``, ``maximize``,
    ``capturable``, ``differentiable``, ``fused`` and a tensor ``lr`` raise ``ValueError``; ``foreach`` is accepted and ignored."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0, amsgrad: bool = False,
                 **kwargs):
        if isinstance(lr, Tensor):
            raise ValueError("gscodec_studio_amd.optimizers: a tensor lr is not supported (pass a float)")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, **kwargs)

    def add_param_group(self, param_group: dict) -> None:
        _check_group({**self.defaults, **param_group})  # (before torch appends it)
        super().add_param_group(param_group)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        _validate(self, False, None)
        entries: List = []
        _collect(self, False, None, entries)
        _launch(entries)
        return loss


class SelectiveAdam(torch.optim.Adam):
    """The reference's ``gsplat.optimizers.SelectiveAdam``: Adam without bias correction that updates only the rows whose
    ``visibility`` (bool / uint8 [N]) is set; one tensor per group, ``M = numel // N`` floats per row.  All groups in one launch."""

    def __init__(self, params, eps, betas):
        super().__init__(params=params, eps=eps, betas=betas)

    @torch.no_grad()
    def step(self, visibility):
        _validate(self, True, visibility)
        entries: List = []
        _collect(self, True, visibility, entries)
        _launch(entries)


def step_all(optimizers: Union[Dict[str, torch.optim.Optimizer], Iterable[torch.optim.Optimizer]], visibility: Optional[Tensor] = None,
             zero_grad: bool = True) -> None:
    """Step every optimizer in ONE ``gs_adam_multi`` call (per device), then ``zero_grad(set_to_none=True)`` each of them.

    ``optimizers``: a dict (the trainer's ``self.optimizers``) or an iterable of ``Adam``, ``torch.optim.Adam`` (supported
    settings; its ``step`` state is advanced exactly as its own ``step()`` would), ``SelectiveAdam`` (needs ``visibility``) and
    ``SparseAdam`` / ``torch.optim.SparseAdam`` (sparse gradients: planned together over all of them, one sort and one
    ``gs_sparse_adam_multi`` call per index list).
    Parameters whose ``grad`` is None are skipped.  Every optimizer is checked before any state changes.  The optimizers' own
    ``step`` hooks do not run (their ``step`` is not called)."""
    opts = list(optimizers.values()) if isinstance(optimizers, dict) else list(optimizers)
    kinds, sparse_opts = [], []
    for opt in opts:
        if isinstance(opt, torch.optim.SparseAdam):
            sparse_opts.append(opt)
        elif isinstance(opt, SelectiveAdam):
            kinds.append((opt, True))
        elif isinstance(opt, torch.optim.Adam):
            kinds.append((opt, False))
        else:
            raise TypeError(f"step_all: {type(opt).__name__} is not an Adam / SelectiveAdam / SparseAdam optimizer")
    for opt, sel in kinds:
        _validate(opt, sel, visibility)
    for opt in sparse_opts:
        _sparse.validate(opt)
    entries: List = []
    with torch.no_grad():
        for opt, sel in kinds:
            _collect(opt, sel, visibility, entries)
        _launch(entries)
        _sparse.step_sparse(sparse_opts)
    for opt in opts:
        opt._opt_called = True  # what the optimizer's own step() wrapper records (an LR scheduler checks it)
        if zero_grad:
            opt.zero_grad(set_to_none=True)


from . import sparse as _sparse  # noqa: E402  (it uses _check_state / _param_name above)
from .sparse import SparseAdam, sparsify_grads  # noqa: E402


def visibility_mask(meta: dict, n: Optional[int] = None) -> Tensor:
    """bool [N]: the gaussians that ``rasterization()`` saw in any camera -- ``(radii > 0).any(0)`` for the dense meta (through
    the ``gs_dp_visibility`` kernel), ``gaussian_ids`` scattered for the packed meta; what the trainers pass to
    ``SelectiveAdam.step`` (``simple_trainer.py``'s ``visible_adam`` branch)."""
    radii = meta["radii"]
    gids = meta.get("gaussian_ids")
    if gids is not None:  # packed: radii [nnz], one entry per (camera, gaussian) pair
        if n is None:
            raise ValueError("visibility_mask: the packed meta needs n (the number of gaussians)")
        vis = torch.zeros(n, dtype=torch.bool, device=gids.device)
        vis[gids] = True
        return vis
    W._require_gpu(radii, "visibility_mask")
    N = radii.shape[-1]
    if n is not None and n != N:
        raise ValueError(f"visibility_mask: meta['radii'] covers {N} gaussians, n = {n}")
    r2 = radii.reshape(-1, N).to(torch.int32).contiguous()  # [C, N]
    vis = torch.empty(N, dtype=torch.uint8, device=radii.device)
    if N > 0:
        with W._device_of(radii):
            W.B.call("gs_dp_visibility", r2.shape[0], N, N, W.B.ptr(r2), W.B.ptr(vis), W._stream(radii))
    return vis.view(torch.bool)
