"""The operations the densification strategies are made of (counterpart of the reference's ``gsplat/strategy/ops.py``).

Three of them run on every training step and are one HIP launch each: ``densify_stats`` (``DefaultStrategy._update_state``,
``gs_densify_stats``), ``inject_noise_to_position`` (``MCMCStrategy``, ``gs_inject_noise``) and ``stg_freeze_grads``
(``STG_Strategy``'s omega / rotation freeze, ``gs_stg_freeze_grads``).  ``stg_omega_mask`` (``gs_stg_omega_mask``) builds the mask the
freeze applies.  ``relocate`` / ``sample_add`` go through ``relocation.compute_relocation`` (``gs_relocation``).  The others change the SET of gaussians every hundred steps or
so and are torch indexing: one gather / ``cat`` per tensor.

All of them replace ``params[name]`` by a new ``Parameter`` and move the optimizer's state to it, for ``torch.optim.Adam``,
``optimizers.Adam`` and ``optimizers.SelectiveAdam`` alike (the state's ``step`` is a CPU scalar and stays as it is).  Parameter names
containing ``"decoder"`` are skipped, and a parameter without an optimizer must not require a gradient.  Random draws come from torch's
global generator on the parameters' device, one draw per call with the reference's shapes, so seeded runs are reproducible.
CPU tensors are refused: there is no CPU fallback.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Union

import numpy as np
import torch
from torch import Tensor

from .. import _backend as B
from .._wrapper import _device_of, _require_gpu, _stream
from ..relocation import compute_relocation

Params = Union[Dict[str, torch.nn.Parameter], torch.nn.ParameterDict]

__all__ = ["duplicate", "split", "remove", "reset_opa", "relocate", "sample_add", "inject_noise_to_position", "densify_stats",
           "stg_omega_mask", "stg_freeze_grads"]


@torch.no_grad()
def _multinomial_sample(weights: Tensor, n: int, replacement: bool = True) -> Tensor:
    """``n`` indices drawn with probabilities proportional to ``weights [M]``: ``torch.multinomial`` up to its limit of 2^24
    categories, ``numpy.random.choice`` (numpy's global generator) above it."""
    m = weights.size(0)
    if m <= 2**24:
        return torch.multinomial(weights, n, replacement=replacement)
    p = (weights / weights.sum()).detach().cpu().numpy()
    idx = np.random.choice(m, size=n, p=p, replace=replacement)
    return torch.from_numpy(idx).to(weights.device)


@torch.no_grad()
def _update_param_with_optimizer(param_fn: Callable[[str, Tensor], Tensor], optimizer_fn: Callable[[str, Tensor], Tensor], params: Params,
                                 optimizers: Dict[str, torch.optim.Optimizer], names: Optional[List[str]] = None) -> None:
    """Replace ``params[name]`` by ``param_fn(name, param)`` and every tensor of its optimizer state except ``step`` by
    ``optimizer_fn(key, value)``, re-keyed to the new parameter.  ``names`` defaults to every parameter whose name does not
    contain ``"decoder"``."""
    if names is None:
        names = [k for k in params.keys() if "decoder" not in k]
    for name in names:
        old = params[name]
        new = param_fn(name, old)
        params[name] = new
        opt = optimizers[name] if name in optimizers else None
        if opt is None:
            assert not old.requires_grad, (f"Optimizer for {name} is not found, but the parameter is trainable."
                                           f"Got requires_grad={old.requires_grad}")
            continue
        st = opt.state.pop(old, {})
        for key in list(st.keys()):
            if key != "step":
                st[key] = optimizer_fn(key, st[key])
        for group in opt.param_groups:
            group["params"] = [new]
        opt.state[new] = st


def _param(t: Tensor, like: Tensor) -> torch.nn.Parameter:
    return torch.nn.Parameter(t, requires_grad=like.requires_grad)


def _zeros_rows(n: int, like: Tensor) -> Tensor:
    return torch.zeros((n, *like.shape[1:]), dtype=like.dtype, device=like.device)


@torch.no_grad()
def duplicate(params: Params, optimizers: Dict[str, torch.optim.Optimizer], state: Dict[str, Tensor], mask: Tensor) -> None:
    """Append a copy of every gaussian of ``mask`` (bool [N]): optimizer state of the copies zero, ``state`` tensors copied."""
    _require_gpu(mask, "strategy.ops.duplicate")
    sel = torch.where(mask)[0]
    _update_param_with_optimizer(lambda name, p: _param(torch.cat([p, p[sel]]), p),
                                 lambda key, v: torch.cat([v, _zeros_rows(len(sel), v)]), params, optimizers)
    for k, v in state.items():
        if isinstance(v, Tensor):
            state[k] = torch.cat((v, v[sel]))


@torch.no_grad()
def split(params: Params, optimizers: Dict[str, torch.optim.Optimizer], state: Dict[str, Tensor], mask: Tensor,
          revised_opacity: bool = False) -> None:
    """Replace every gaussian of ``mask`` by two, appended behind the others: means drawn from the parent (``mean + R diag(s) z``, one
    ``torch.randn(2, n, 3)``), scales / 1.6, and with ``revised_opacity`` the opacity ``1 - sqrt(1 - o)`` of arXiv:2404.06109."""
    _require_gpu(mask, "strategy.ops.split")
    device = mask.device
    sel, rest = torch.where(mask)[0], torch.where(~mask)[0]
    scales = torch.exp(params["scales"][sel])
    q = torch.nn.functional.normalize(params["quats"][sel], dim=-1)
    w, x, y, z = q.unbind(-1)
    rot = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                       2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                       2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(-1, 3, 3)
    samples = torch.einsum("nij,nj,bnj->bni", rot, scales, torch.randn(2, len(scales), 3, device=device))  # [2, n, 3]

    def param_fn(name: str, p: Tensor) -> Tensor:
        twice = [2] + [1] * (p.dim() - 1)
        if name == "means":
            new = (p[sel] + samples).reshape(-1, 3)
        elif name == "scales":
            new = torch.log(scales / 1.6).repeat(2, 1)
        elif name == "opacities" and revised_opacity:
            new = torch.logit(1.0 - torch.sqrt(1.0 - torch.sigmoid(p[sel]))).repeat(twice)
        else:
            new = p[sel].repeat(twice)
        return _param(torch.cat([p[rest], new]), p)

    _update_param_with_optimizer(param_fn, lambda key, v: torch.cat([v[rest], _zeros_rows(2 * len(sel), v)]), params, optimizers)
    for k, v in state.items():
        if isinstance(v, Tensor):
            state[k] = torch.cat((v[rest], v[sel].repeat([2] + [1] * (v.dim() - 1))))


@torch.no_grad()
def remove(params: Params, optimizers: Dict[str, torch.optim.Optimizer], state: Dict[str, Tensor], mask: Tensor) -> None:
    """Drop every gaussian of ``mask`` (bool [N])."""
    _require_gpu(mask, "strategy.ops.remove")
    keep = torch.where(~mask)[0]
    _update_param_with_optimizer(lambda name, p: _param(p[keep], p), lambda key, v: v[keep], params, optimizers)
    for k, v in state.items():
        if isinstance(v, Tensor):
            state[k] = v[keep]


@torch.no_grad()
def reset_opa(params: Params, optimizers: Dict[str, torch.optim.Optimizer], state: Dict[str, Tensor], value: float) -> None:
    """Clamp the opacities to at most ``value`` (after the sigmoid) and zero their optimizer state."""
    _require_gpu(params["opacities"], "strategy.ops.reset_opa")
    ceiling = torch.logit(torch.tensor(value)).item()  # (a CPU scalar: no device synchronisation)

    def param_fn(name: str, p: Tensor) -> Tensor:
        if name != "opacities":
            raise ValueError(f"Unexpected parameter name: {name}")
        return _param(torch.clamp(p, max=ceiling), p)

    _update_param_with_optimizer(param_fn, lambda key, v: torch.zeros_like(v), params, optimizers, names=["opacities"])


def _relocation_of(params: Params, sampled: Tensor, binoms: Tensor, min_opacity: float):
    """New (clamped) opacities and scales of the sampled gaussians, each standing for 1 + (times it was drawn) copies."""
    opacities = torch.sigmoid(params["opacities"])
    new_opacities, new_scales = compute_relocation(
        opacities=opacities[sampled].flatten(), scales=torch.exp(params["scales"])[sampled],
        ratios=torch.bincount(sampled)[sampled] + 1, binoms=binoms)
    eps = torch.finfo(torch.float32).eps
    return torch.clamp(new_opacities, max=1.0 - eps, min=min_opacity), new_scales


@torch.no_grad()
def relocate(params: Params, optimizers: Dict[str, torch.optim.Optimizer], state: Dict[str, Tensor], mask: Tensor, binoms: Tensor,
             min_opacity: float = 0.005) -> None:
    """Move the dead gaussians (``mask``) onto live ones drawn with probability proportional to their opacity (one
    ``torch.multinomial``); the drawn gaussians get the relocation opacity and scale, the dead ones become copies of them, and the
    optimizer state (and ``state``) of the drawn rows is zeroed.  The number of gaussians does not change."""
    _require_gpu(mask, "strategy.ops.relocate")
    dead = mask.nonzero(as_tuple=True)[0]
    alive = (~mask).nonzero(as_tuple=True)[0]
    probs = torch.sigmoid(params["opacities"])[alive].flatten()
    sampled = alive[_multinomial_sample(probs, len(dead), replacement=True)]
    new_opacities, new_scales = _relocation_of(params, sampled, binoms, min_opacity)

    def param_fn(name: str, p: Tensor) -> Tensor:
        if name == "opacities":
            p[sampled] = torch.logit(new_opacities).reshape(p[sampled].shape)
        elif name == "scales":
            p[sampled] = torch.log(new_scales)
        p[dead] = p[sampled]
        return _param(p, p)

    def optimizer_fn(key: str, v: Tensor) -> Tensor:
        v[sampled] = 0
        return v

    _update_param_with_optimizer(param_fn, optimizer_fn, params, optimizers)
    for k, v in state.items():
        if isinstance(v, Tensor):
            v[sampled] = 0


@torch.no_grad()
def sample_add(params: Params, optimizers: Dict[str, torch.optim.Optimizer], state: Dict[str, Tensor], n: int, binoms: Tensor,
               min_opacity: float = 0.005) -> None:
    """Append ``n`` gaussians: copies of gaussians drawn with probability proportional to their opacity (one ``torch.multinomial``),
    source and copy both with the relocation opacity and scale; optimizer state (and ``state``) of the new rows zero."""
    _require_gpu(params["means"], "strategy.ops.sample_add")
    probs = torch.sigmoid(params["opacities"]).flatten()
    sampled = _multinomial_sample(probs, n, replacement=True)
    new_opacities, new_scales = _relocation_of(params, sampled, binoms, min_opacity)

    def param_fn(name: str, p: Tensor) -> Tensor:
        if name == "opacities":
            p[sampled] = torch.logit(new_opacities).reshape(p[sampled].shape)
        elif name == "scales":
            p[sampled] = torch.log(new_scales)
        return _param(torch.cat([p, p[sampled]]), p)

    _update_param_with_optimizer(param_fn, lambda key, v: torch.cat([v, _zeros_rows(len(sampled), v)]), params, optimizers)
    for k, v in state.items():
        if isinstance(v, Tensor):
            state[k] = torch.cat((v, _zeros_rows(len(sampled), v)))


def _as_f32(t: Tensor, what: str, name: str) -> Tensor:
    if t.dtype != torch.float32:
        raise RuntimeError(f"{what}: {name} must be float32, got {t.dtype}")
    return t


@torch.no_grad()
def inject_noise_to_position(params: Params, optimizers: Dict[str, torch.optim.Optimizer], state: Dict[str, Tensor],
                             scaler: float) -> None:
    """``means += Sigma * (noise * g(1 - sigmoid(opacities)) * scaler)`` in place, ``noise = torch.randn_like(means)`` (one draw),
    ``g(x) = 1 / (1 + exp(-100 (x - 0.995)))``, ``Sigma`` the covariance from the raw ``quats`` and log ``scales``: the random draw
    plus one ``gs_inject_noise`` launch."""
    what = "strategy.ops.inject_noise_to_position"
    means = params["means"]
    _require_gpu(means, what)
    N = means.shape[0]
    quats, scales, opac = (params[k].detach() for k in ("quats", "scales", "opacities"))
    for t, name, shape in ((means, "means", (N, 3)), (quats, "quats", (N, 4)), (scales, "scales", (N, 3))):
        _as_f32(t, what, name)
        if tuple(t.shape) != shape or t.device != means.device:
            raise RuntimeError(f"{what}: {name} is {tuple(t.shape)} on {t.device}, expected {shape} on {means.device}")
    _as_f32(opac, what, "opacities")
    if opac.numel() != N or opac.device != means.device:
        raise RuntimeError(f"{what}: opacities is {tuple(opac.shape)} on {opac.device}, expected [{N}] or [{N}, 1] on {means.device}")
    if not means.is_contiguous():
        raise RuntimeError(f"{what}: means must be contiguous (it is updated in place)")
    noise = torch.randn_like(means)
    quats, scales, opac, noise = quats.contiguous(), scales.contiguous(), opac.reshape(N).contiguous(), noise.contiguous()
    with _device_of(means):
        B.call("gs_inject_noise", N, B.ptr(means), B.ptr(quats), B.ptr(scales), B.ptr(opac), B.ptr(noise), float(scaler), _stream(means))


def _grad_rows(grad: Tensor):
    """(tensor whose storage the kernel reads, floats between consecutive rows of 2) for a [..., 2] float32 gradient: contiguous,
    or a column pair of a wider row-major buffer (the gradient rows of the compositing backward) -- otherwise a contiguous copy."""
    if grad.stride(-1) == 1:
        stride = grad.stride(-2) if grad.dim() >= 2 else 2
        ok = stride >= 2
        expect = stride
        for d in range(grad.dim() - 2, -1, -1):  # rows evenly spaced over all the leading dimensions
            if grad.shape[d] > 1 and grad.stride(d) != expect:
                ok = False
            expect *= grad.shape[d]
        if ok:
            return grad, int(stride)
    return grad.contiguous(), 2


@torch.no_grad()
def densify_stats(grad: Tensor, radii: Tensor, gaussian_ids: Optional[Tensor], width: int, height: int, n_cameras: int,
                  grad2d: Tensor, count: Tensor, radii_state: Optional[Tensor] = None) -> None:
    """Accumulate the running statistics of ``DefaultStrategy`` in place, in one ``gs_densify_stats`` launch and without a host
    synchronisation.

    ``grad``: the image-plane gradient of ``means2d``, ``[C, N, 2]`` (``gaussian_ids`` None) or ``[nnz, 2]`` with ``gaussian_ids
    int64 [nnz]``; ``radii``: ``[C, N]`` / ``[nnz]`` integer.  For every (camera, gaussian) pair with ``radii > 0``:
    ``grad2d[n] += hypot(gx * width / 2 * n_cameras, gy * height / 2 * n_cameras)``, ``count[n] += 1`` and, with ``radii_state``,
    ``radii_state[n] = max(radii_state[n], radii / max(width, height))``.

    One deliberate difference from the reference (``strategy/default.py:255-261``): with several cameras its indexed assignment
    ``state["radii"][gs_ids] = maximum(state["radii"][gs_ids], ...)`` keeps whichever duplicate index wins the scatter; this
    computes the true maximum over the cameras (what its own comment asks for).  With one camera the two agree.  The unpacked form
    uses no atomics and is bit-identical from run to run; the packed form sums with float atomics."""
    what = "strategy.ops.densify_stats"
    _require_gpu(grad, what)
    N = grad2d.shape[0]
    packed = gaussian_ids is not None
    _as_f32(grad, what, "grad")
    for t, name in ((grad2d, "grad2d"), (count, "count"), (radii_state, "radii_state")):
        if t is None:
            continue
        _as_f32(t, what, name)
        if t.shape != (N,) or not t.is_contiguous() or t.device != grad.device:
            raise RuntimeError(f"{what}: {name} must be a contiguous [{N}] tensor on {grad.device}")
    if grad.shape[-1] != 2:
        raise RuntimeError(f"{what}: grad must end in a dimension of 2, got {tuple(grad.shape)}")
    if packed:
        nnz, C = grad.shape[0], max(int(n_cameras), 1)
        if grad.dim() != 2 or radii.shape != (nnz,) or gaussian_ids.shape != (nnz,) or gaussian_ids.dtype != torch.int64:
            raise RuntimeError(f"{what}: packed form needs grad [nnz, 2], radii [nnz], gaussian_ids int64 [nnz]; got "
                               f"{tuple(grad.shape)}, {tuple(radii.shape)}, {tuple(gaussian_ids.shape)} {gaussian_ids.dtype}")
        gaussian_ids = gaussian_ids.contiguous()
    else:
        nnz = 0
        if grad.dim() != 3 or grad.shape[1] != N or radii.shape != grad.shape[:2]:
            raise RuntimeError(f"{what}: unpacked form needs grad [C, {N}, 2] and radii [C, {N}]; got {tuple(grad.shape)}, "
                               f"{tuple(radii.shape)}")
        C = grad.shape[0]
    if radii.device != grad.device or (packed and gaussian_ids.device != grad.device):
        raise RuntimeError(f"{what}: radii / gaussian_ids must be on {grad.device}")
    radii = radii.to(torch.int32).contiguous()
    src, stride = _grad_rows(grad)
    if N == 0 or C == 0:
        return
    with _device_of(grad):
        B.call("gs_densify_stats", C, N, nnz, B.ptr(src), stride, B.ptr(radii), B.ptr(gaussian_ids), width / 2.0 * n_cameras,
               height / 2.0 * n_cameras, float(max(width, height)), B.ptr(grad2d), B.ptr(count), B.ptr(radii_state), _stream(grad))


@torch.no_grad()
def stg_omega_mask(motion: Tensor, scales: Tensor, opacities: Tensor, omega: Tensor, motion_min: float = 0.3, scale_min: float = 0.2,
                   scale_max: float = 0.6, opacity_min: float = 0.7):
    """The mask of ``STG_Strategy._zero_omegabymotion`` and the masked omega, from the raw parameters in one ``gs_stg_omega_mask``
    launch: ``mask = sum|motion[:, 0:3]| > motion_min & scale_min < max exp(scales) < scale_max & sigmoid(opacities) > opacity_min``
    (bool ``[N, 1]``) and ``omega_new = mask.float() * omega`` (``[N, 4]``).  ``motion`` is ``[N, M >= 3]`` and read in place through
    its row stride; ``opacities`` is ``[N]`` or ``[N, 1]``."""
    what = "strategy.ops.stg_omega_mask"
    _require_gpu(omega, what)
    motion, scales, opacities, omega = motion.detach(), scales.detach(), opacities.detach(), omega.detach()
    N = omega.shape[0]
    if motion.dim() != 2 or motion.shape[0] != N or motion.shape[1] < 3:
        raise RuntimeError(f"{what}: motion is {tuple(motion.shape)}, expected [{N}, >= 3]")
    for t, name, shape in ((scales, "scales", (N, 3)), (omega, "omega", (N, 4))):
        if tuple(t.shape) != shape:
            raise RuntimeError(f"{what}: {name} is {tuple(t.shape)}, expected {shape}")
    if opacities.numel() != N:
        raise RuntimeError(f"{what}: opacities is {tuple(opacities.shape)}, expected [{N}] or [{N}, 1]")
    for t, name in ((motion, "motion"), (scales, "scales"), (opacities, "opacities"), (omega, "omega")):
        _as_f32(t, what, name)
        if t.device != omega.device:
            raise RuntimeError(f"{what}: {name} is on {t.device}, omega on {omega.device}")
    if motion.stride(1) != 1 or (N > 1 and motion.stride(0) < 3):
        motion = motion.contiguous()
    stride = motion.stride(0) if N > 1 else motion.shape[1]
    scales, opacities, omega = scales.contiguous(), opacities.reshape(N).contiguous(), omega.contiguous()
    mask = torch.empty((N, 1), dtype=torch.bool, device=omega.device)
    omega_new = torch.empty_like(omega)
    with _device_of(omega):
        B.call("gs_stg_omega_mask", N, B.ptr(motion), int(stride), B.ptr(scales), B.ptr(opacities), B.ptr(omega), float(motion_min),
               float(scale_min), float(scale_max), float(opacity_min), B.ptr(mask), B.ptr(omega_new), _stream(omega))
    return mask, omega_new


@torch.no_grad()
def stg_freeze_grads(mask: Tensor, omega_grad: Tensor, quats_grad: Tensor) -> None:
    """``omega_grad *= mask`` and ``quats_grad *= ~mask`` row by row, IN PLACE, in one ``gs_stg_freeze_grads`` launch: no allocation,
    no host synchronisation.  ``mask``: bool (or uint8 0 / 1) ``[N]`` / ``[N, 1]``; the gradients: contiguous float32 ``[N, 4]``.
    The rows are multiplied by 0.0 or 1.0, so a non-finite gradient stays non-finite under a zero, as in ``grad * mask``."""
    what = "strategy.ops.stg_freeze_grads"
    for t, name in ((omega_grad, "omega.grad"), (quats_grad, "quats.grad")):
        if not isinstance(t, Tensor):  # (what the reference's `None * mask` raises)
            raise TypeError(f"{what}: {name} is {type(t).__name__}, not a tensor -- the freeze runs after backward()")
    _require_gpu(omega_grad, what)
    N = omega_grad.shape[0]
    if mask.dtype not in (torch.bool, torch.uint8) or mask.numel() != N or mask.device != omega_grad.device or not mask.is_contiguous():
        raise RuntimeError(f"{what}: mask must be a contiguous bool / uint8 tensor of {N} elements on {omega_grad.device}, got "
                           f"{mask.dtype} {tuple(mask.shape)} on {mask.device}")
    for t, name in ((omega_grad, "omega.grad"), (quats_grad, "quats.grad")):
        _as_f32(t, what, name)
        if tuple(t.shape) != (N, 4) or not t.is_contiguous() or t.device != omega_grad.device:
            raise RuntimeError(f"{what}: {name} must be a contiguous [{N}, 4] tensor on {omega_grad.device} (it is scaled in place), "
                               f"got {tuple(t.shape)} on {t.device}")
    with _device_of(omega_grad):
        B.call("gs_stg_freeze_grads", N, B.ptr(mask), B.ptr(omega_grad), B.ptr(quats_grad), _stream(omega_grad))
