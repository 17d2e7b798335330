"""SparseAdam for the trainers' ``--sparse_grad`` mode, stepped by one HIP kernel (``gs_sparse_adam_multi``, csrc/optim.hip).

* ``SparseAdam`` -- a drop-in ``torch.optim.SparseAdam`` (same constructor, same state: ``step`` a Python int, ``exp_avg``,
  ``exp_avg_sq``; ``step`` advances for every parameter that has a gradient, an empty one included), so ``state_dict`` /
  ``load_state_dict`` work both ways with torch's.  Only the rows that occur in the gradient's indices are read or written.
* ``sparsify_grads(params, gaussian_ids, coalesced)`` -- the trainer's loop that turns the dense gradients of the other splat
  tensors into COO tensors over ``gaussian_ids`` (``examples/simple_trainer.py``, "Turn Gradients into Sparse Tensor").
* ``step_sparse(optimizers)`` -- what ``SparseAdam.step`` and ``step_all`` share: the gradients of all the optimizers are grouped
  by their index list (same device, rows, nnz, ``is_coalesced()`` and ``_indices()`` storage), every group is sorted ONCE
  (``gs_sort_pairs_u64_i32`` over (ids, 0 .. nnz - 1) and the bits of ``rows - 1``: stable, so duplicates are summed in ascending
  position; no sort for a coalesced gradient) and stepped by ONE ``gs_sparse_adam_multi`` call.  Gradients whose indices do not
  share storage fall into groups of their own: correct, only slower.

Index storage.  ``torch.sparse_coo_tensor(indices=ids[None], ...)`` keeps ``ids``' storage (checked with torch 2.10 for ROCm, on
the CPU and on an MI355X, with ``is_coalesced`` unset, False and True: ``_indices().data_ptr() == ids.data_ptr()``), and so does
autograd's accumulation into ``.grad`` of a sparse gradient nobody else holds: after ``rasterization(packed=True,
sparse_grad=True)`` and a backward, the ``.grad`` of ``means``, ``quats`` and ``scales`` still point at ``info["gaussian_ids"]``.
So those and the ones ``sparsify_grads`` builds over the same ``gaussian_ids`` land in one group.  A gradient that passes through
another autograd node on its way (``scales`` through ``exp``: a sparse-times-dense product) gets index storage of its own, and a
``means`` gradient that also receives the dense share of the SH view directions arrives dense and is sparsified with the rest.

There is no fallback to torch's sparse code: a gradient the kernel cannot step raises, before anything is mutated.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Iterable, List, Optional, Tuple

import torch
from torch import Tensor

from .. import _backend as B
from .. import _wrapper as W

_PREFIX = "gscodec_studio_amd.optimizers"
_DESC_FIELDS = ("param", "exp_avg", "exp_avg_sq", "values", "row_width", "one_minus_beta1", "one_minus_beta2", "neg_step_size", "eps")
_DESC: List[type] = []


def sparse_adam_desc_class() -> type:
    """The ctypes class of ``gs_sparse_adam_desc``, derived from the header and checked once against the library's own layout
    (``gs_sparse_adam_desc_layout``) before the first descriptor is built."""
    if not _DESC:
        _DESC.append(B.guarded_struct("gs_sparse_adam_desc", "gs_sparse_adam_desc_layout", _DESC_FIELDS))
    return _DESC[0]


def sparse_adam_scalars(lr: float, beta1: float, beta2: float, step: int) -> Tuple[float, float, float]:
    """(1 - beta1, 1 - beta2, -step_size) of ``torch.optim._functional.sparse_adam`` at ``step`` (already advanced), in double as
    torch computes them; the descriptor rounds them to float as torch's scalar-times-tensor kernels do."""
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    return 1 - beta1, 1 - beta2, -(lr * math.sqrt(bias_correction2) / bias_correction1)


def sparse_adam_desc(param: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, values: Tensor, row_width: int, lr: float, beta1: float,
                     beta2: float, eps: float, step: int):
    """One ``gs_sparse_adam_desc`` (``step`` = the advanced step counter)."""
    d = sparse_adam_desc_class()()
    d.param, d.exp_avg, d.exp_avg_sq, d.values = param.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), values.data_ptr()
    d.row_width = row_width
    d.one_minus_beta1, d.one_minus_beta2, d.neg_step_size = sparse_adam_scalars(lr, beta1, beta2, step)
    d.eps = eps
    return d


def sparse_adam_multi(descs, nnz: int, sorted_ids: Tensor, perm: Optional[Tensor], rows: int, like: Tensor) -> None:
    """Launch ``gs_sparse_adam_multi`` over ``descs`` (tensors on ``like``'s device) on the current stream."""
    if not descs or nnz == 0:
        return
    table = (sparse_adam_desc_class() * len(descs))(*descs)
    with W._device_of(like):
        B.call("gs_sparse_adam_multi", len(descs), ctypes.addressof(table), nnz, B.ptr(sorted_ids), B.ptr(perm), rows, W._stream(like))


def sort_ids(ids: Tensor, rows: int) -> Tuple[Tensor, Optional[Tensor]]:
    """(sorted ids, perm) of int64 ``ids`` [nnz] in [0, rows): a stable sort on (id, position); perm None where nothing moves."""
    nnz = ids.numel()
    bits = (rows - 1).bit_length()
    if bits == 0 or nnz < 2:
        return ids, None
    iota = torch.arange(nnz, dtype=torch.int32, device=ids.device)
    sorted_ids, perm = torch.empty_like(ids), torch.empty_like(iota)
    with W._device_of(ids):
        temp = torch.empty(int(B.query("gs_sort_temp_bytes", nnz)), dtype=torch.uint8, device=ids.device)
        B.call("gs_sort_pairs_u64_i32", nnz, B.ptr(ids), B.ptr(iota), B.ptr(sorted_ids), B.ptr(perm), 0, bits, B.ptr(temp), temp.numel(),
               W._stream(ids))
    return sorted_ids, perm


def _check_group(group: dict) -> None:
    """Refuse the torch.optim.SparseAdam settings the kernel does not implement."""
    if isinstance(group.get("lr"), Tensor):
        raise ValueError(f"{_PREFIX}: a tensor lr is not supported (pass a float)")
    if any(isinstance(b, Tensor) for b in group.get("betas", ())):
        raise ValueError(f"{_PREFIX}: tensor betas are not supported (pass floats)")
    if group.get("maximize", False):
        raise ValueError(f"{_PREFIX}: maximize=True is not supported")


def _check_param(opt: torch.optim.Optimizer, p: Tensor, group: dict, gi: int, pi: int) -> None:
    from . import _check_state, _param_name

    g = p.grad
    what = _param_name(group, gi, pi)
    if not g.is_sparse:
        raise RuntimeError("SparseAdam does not support dense gradients, please consider Adam instead")
    for t, kind in ((p, "parameter"), (g, "gradient")):
        if t.dtype != torch.float32:
            raise RuntimeError(f"{_PREFIX}: {kind} of {what} is {t.dtype}; only float32 is supported")
    if g.sparse_dim() != 1:
        raise RuntimeError(f"{_PREFIX}: gradient of {what} has {g.sparse_dim()} sparse dimensions; only 1 (the rows) is supported")
    if g.shape != p.shape or g.device != p.device:
        raise RuntimeError(f"{_PREFIX}: gradient of {what} does not match the parameter's shape / device")
    if not p.is_cuda:
        raise RuntimeError(f"{_PREFIX}: parameter of {what} is on {p.device}; the HIP step needs a GPU tensor")
    if not p.is_contiguous():
        raise RuntimeError(f"{_PREFIX}: parameter of {what} is not contiguous")
    width = math.prod(p.shape[1:])
    if p.shape[0] * width >= 1 << 32 or g._nnz() * width >= 1 << 32 or g._nnz() >= 1 << 31:
        raise RuntimeError(f"{_PREFIX}: {what}: rows * row_width and nnz * row_width must be < 2^32, nnz < 2^31")
    _check_state(opt, p, what)


def validate(opt: torch.optim.Optimizer) -> None:
    """Every check of a sparse step, before anything is mutated."""
    for gi, group in enumerate(opt.param_groups):
        _check_group(group)
        for pi, p in enumerate(group["params"]):
            if p.grad is not None:
                _check_param(opt, p, group, gi, pi)


def _init_state(opt: torch.optim.Optimizer, p: Tensor) -> dict:
    st = opt.state[p]
    if len(st) == 0:  # torch.optim.SparseAdam's lazy state: a Python int step
        st["step"] = 0
        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
    return st


def step_sparse(optimizers: Iterable[torch.optim.Optimizer]) -> None:
    """Advance the step counters as ``torch.optim.SparseAdam.step`` would and step every parameter that has a (validated) sparse
    gradient: one sort and one launch per index list, over all the optimizers."""
    plans: Dict[tuple, List] = {}
    for opt in optimizers:
        for group in opt.param_groups:
            lr, eps = group["lr"], group["eps"]
            beta1, beta2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = _init_state(opt, p)
                st["step"] += 1
                g = p.grad
                nnz, width = g._nnz(), math.prod(p.shape[1:])
                if nnz == 0 or p.numel() == 0:  # (torch: "Skip update for empty grad")
                    continue
                idx = g._indices()
                key = (p.device, p.shape[0], nnz, g.is_coalesced(), idx.data_ptr(), idx.stride())
                values = g._values()
                values = values if values.is_contiguous() else values.contiguous()
                desc = sparse_adam_desc(p, st["exp_avg"], st["exp_avg_sq"], values, width, lr, beta1, beta2, eps, st["step"])
                plans.setdefault(key, []).append((idx, desc, values))  # (values: kept alive to the launch)
    for (_, rows, nnz, coalesced, _, _), items in plans.items():
        ids = items[0][0][0]
        ids = ids if ids.is_contiguous() else ids.contiguous()
        sorted_ids, perm = (ids, None) if coalesced else sort_ids(ids, rows)
        sparse_adam_multi([d for _, d, _ in items], nnz, sorted_ids, perm, rows, ids)


class SparseAdam(torch.optim.SparseAdam):
    """``torch.optim.SparseAdam`` stepped by the HIP kernel (``gs_sparse_adam_multi``): the same constructor, state layout and step
    semantics.  Gradients: COO with one sparse dimension (the rows), float32, on the GPU.  ``maximize=True`` and a tensor ``lr``
    raise ``ValueError``.  Duplicate indices are summed in ascending position before the update."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, maximize: bool = False):
        if isinstance(lr, Tensor):
            raise ValueError(f"{_PREFIX}: a tensor lr is not supported (pass a float)")
        super().__init__(params, lr=lr, betas=betas, eps=eps, maximize=maximize)

    def add_param_group(self, param_group: dict) -> None:
        _check_group({**self.defaults, **param_group})  # (before torch appends it)
        super().add_param_group(param_group)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        validate(self)
        step_sparse([self])
        return loss


def sparsify_grads(params, gaussian_ids: Tensor, coalesced: bool = False) -> None:
    """The trainer's loop before the optimizers in ``--sparse_grad`` mode: every dense ``grad`` [N, ...] of ``params`` (a dict,
    ``ParameterDict`` or iterable of tensors) becomes ``torch.sparse_coo_tensor(gaussian_ids[None], grad[gaussian_ids], size,
    is_coalesced=coalesced)``; ``None`` and already sparse gradients are left alone.  ``coalesced``: the trainer's
    ``len(Ks) == 1`` (one camera: ``gaussian_ids`` ascending and unique).  All of them share ``gaussian_ids``' storage."""
    indices = gaussian_ids[None]  # [1, nnz]
    for p in (params.values() if hasattr(params, "values") else params):
        grad = p.grad
        if grad is None or grad.is_sparse:
            continue
        p.grad = torch.sparse_coo_tensor(indices=indices, values=grad[gaussian_ids], size=p.size(), is_coalesced=coalesced)
