"""Reference arithmetic, the table builder and the named tables shared by tests/test_optimizers_cpu.py and
tests/test_gpu_adam_table.py (gs_adam_multi, csrc/optim.hip).  Plain numpy: no fixtures, no pytest hooks.

* ``dense_f32`` / ``selective_f32``: the kernel's two updates restated in numpy float32, one rounding per operation, from the
  float constants the descriptor carries.  ``dense_f64`` / ``selective_f64``: the same updates in float64 from the double
  hyper-parameters (textbook Adam with its bias corrections; the reference's selective update has none).
* ``build_table(specs, rng)``: host arrays for a list of ``Spec``; every array sits between 8 sentinel floats (bits 0x4B1D4B1D,
  an ordinary finite float) on either side, at the requested byte offset mod 16.
* The named tables: ``EDGE_SIZES``, ``SELECTIVE_WIDTHS``, ``BETAS``, ``SPLIT_COUNTS``, ``MANY_CHUNKS``,
  ``MANY_CHUNKS_ONE_LAUNCH`` and the functions that turn them into spec lists (``named_tables()`` lists them all).

Value ranges: |g| in [1e-3, 1] with n // 20 entries exactly 0, |m| in [1e-3, 1], v in [1e-6, 1] (both log-uniform), |p| in
[0.1, 2]; one tensor per table (``zero_v``) has v = 0 where g = 0, i.e. denom = eps with m != 0: a large, finite update.

Distance of the float32 restatement from the float64 oracle, largest relative error per array over each named table
(|x32 - x64| / |x64|; printed by test_optimizers_cpu.py::test_restatement_against_float64_on_every_named_table).  exp_avg
and p can cancel (m and g of opposite sign; p against a large update), exp_avg_sq cannot; the selective figures carry
1 - float32(beta) against 1 - beta (3e-8 / 0.001 for beta2 = 0.999), the dense ones only the rounding of the double constants:

    table                      p          exp_avg    exp_avg_sq
    edge head 0                6.50e-07   2.61e-04   1.63e-07
    edge head 1                3.99e-06   1.31e-04   1.67e-07
    edge head 2                1.47e-06   1.78e-04   1.55e-07
    edge head 3                6.26e-07   3.10e-04   1.71e-07
    edge mismatched            3.26e-06   2.05e-04   1.55e-07
    selective head 0           1.68e-03   1.09e-02   1.29e-05
    selective head 3           3.06e-04   1.64e-04   1.29e-05
    selective mismatched       1.01e-04   3.85e-04   1.29e-05
    betas                      1.46e-07   2.96e-04   1.57e-07
    split 15                   7.85e-05   1.77e-05   1.29e-05
    split 15 with empty        1.16e-05   5.75e-06   1.29e-05
    split 16                   7.11e-05   5.27e-04   1.29e-05
    split 16 with empty        2.24e-05   4.40e-05   1.29e-05
    split 17                   2.17e-05   1.01e-04   1.29e-05
    split 17 with empty        2.47e-05   3.48e-04   1.29e-05
    split 31                   5.81e-06   1.31e-04   1.29e-05
    split 31 with empty        1.46e-05   7.08e-04   1.29e-05
    split 32                   1.09e-04   6.04e-05   1.29e-05
    split 32 with empty        6.81e-05   3.42e-04   1.29e-05
    split 33                   2.07e-05   4.59e-05   1.29e-05
    split 33 with empty        1.67e-03   3.73e-04   1.29e-05
    split 40                   2.15e-05   5.46e-05   1.29e-05
    split 40 with empty        1.45e-04   2.11e-04   1.29e-05
    many chunks                2.93e-04   2.65e-02   2.15e-07
    many chunks in one launch  9.83e-04   1.27e-02   2.10e-07

The GPU test computes these per descriptor and holds the kernel to twice the restatement's distance plus one float32 ulp.
"""
import dataclasses
from typing import Tuple, Union

import numpy as np

DENSE, SELECTIVE = 0, 1  # GS_ADAM_DENSE / GS_ADAM_SELECTIVE of include/gsplat_hip.h (_wrapper.ADAM_DENSE / ADAM_SELECTIVE)
TABLE_MAX = 16           # GS_ADAM_MULTI_MAX
BLOCK = 256              # GS_BLOCK: a chunk is BLOCK quads of 4 floats

PAD = 8
SENTINEL_BITS = 0x4B1D4B1D
SENTINEL = np.array([SENTINEL_BITS], np.uint32).view(np.float32)[0]
ARRAYS = ("p", "g", "m", "v")
ULP = 2.0 ** -23

f32 = np.float32


# ---------------------------------------------------------------------------
# the two updates, float32 as the kernel rounds them and float64
# ---------------------------------------------------------------------------
def _all_f32(*arrays):
    for a in arrays:
        assert a.dtype == np.float32, a.dtype


def dense_f32(p, g, m, v, c):
    """The dense step of optim.hip's header comment.  c = (one_minus_beta1, beta2, one_minus_beta2, -step_size,
    bias_correction2_sqrt, eps), the float32 values of the descriptor.  Returns the new (p, exp_avg, exp_avg_sq)."""
    _all_f32(p, g, m, v)
    w, b2, w2, neg_step, bc2_sqrt, eps = (f32(x) for x in c)
    if abs(w) < f32(0.5):  # ATen's lerp: the branch is chosen by the weight
        m1 = m + w * (g - m)
    else:
        m1 = g - (g - m) * (f32(1) - w)
    v1 = v * b2
    v1 = v1 + (w2 * g) * g
    denom = np.sqrt(v1) / bc2_sqrt + eps
    p1 = p + neg_step * (m1 / denom)
    _all_f32(p1, m1, v1)
    return p1, m1, v1


def selective_f32(p, g, m, v, vis, row_width, c):
    """gsplat/cuda/csrc/adam.cu:31-40 where vis[e // row_width] is set, the old values elsewhere.  c = (lr, beta1, beta2, eps),
    the float32 values of the descriptor; 1 - beta is formed in float32, as the kernel's host side does."""
    _all_f32(p, g, m, v)
    lr, b1, b2, eps = (f32(x) for x in c)
    w1, w2, neg_lr = f32(1) - b1, f32(1) - b2, -lr
    m1 = b1 * m + w1 * g
    v1 = b2 * v + (w2 * g) * g
    p1 = p + (neg_lr * m1) / (np.sqrt(v1) + eps)
    _all_f32(p1, m1, v1)
    keep = np.repeat(np.asarray(vis) != 0, row_width)
    return np.where(keep, p1, p), np.where(keep, m1, m), np.where(keep, v1, v)


def dense_f64(p, g, m, v, lr, beta1, beta2, eps, step):
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    m1 = beta1 * m + (1.0 - beta1) * g
    v1 = beta2 * v + (1.0 - beta2) * g * g
    m_hat = m1 / (1.0 - beta1 ** step)
    v_hat = v1 / (1.0 - beta2 ** step)
    return p - lr * m_hat / (np.sqrt(v_hat) + eps), m1, v1


def selective_f64(p, g, m, v, vis, row_width, lr, beta1, beta2, eps):
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    m1 = beta1 * m + (1.0 - beta1) * g
    v1 = beta2 * v + (1.0 - beta2) * g * g
    p1 = p - lr * m1 / (np.sqrt(v1) + eps)
    keep = np.repeat(np.asarray(vis) != 0, row_width)
    return np.where(keep, p1, p), np.where(keep, m1, m), np.where(keep, v1, v)


def rel_err(x, ref64):
    """Largest |x - ref| / |ref|; where ref is 0, x has to be 0 too (else inf).  0 for empty arrays."""
    x, ref64 = np.asarray(x, np.float64), np.asarray(ref64, np.float64)
    if x.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.abs(x - ref64) / np.abs(ref64)
    e = np.where(ref64 == 0, np.where(x == 0, 0.0, np.inf), e)
    return float(e.max())


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------
# specs and the table builder
# ---------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Spec:
    mode: int
    n: int                                                   # floats
    offsets: Tuple[int, int, int, int] = (0, 0, 0, 0)        # byte offset mod 16 of p, g, m, v
    row_width: int = 0                                       # selective: n = rows * row_width
    vis: Union[float, str] = 1.0                             # selective: density of set rows, or "alt" (1 0 1 0 ...)
    lr: float = 1e-3
    betas: Tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-15
    step: int = 1                                            # dense: the advanced step counter
    zero_v: bool = False                                     # v = 0 where g = 0

    @property
    def rows(self):
        return self.n // self.row_width if self.mode == SELECTIVE else 0


@dataclasses.dataclass
class Case:
    spec: Spec
    padded: dict            # name -> float32 [PAD + n + PAD], sentinels around the data, data address % 16 = the spec's offset
    vis: np.ndarray         # uint8 [rows] (selective), else None

    def data(self, name):
        return self.padded[name][PAD:PAD + self.spec.n]


def slice_start(address, offset):
    """Floats to skip from a 4-byte aligned ``address`` to reach byte offset ``offset`` mod 16 (0 .. 3)."""
    assert address % 4 == 0 and offset in (0, 4, 8, 12)
    return ((offset - address) % 16) // 4


def _log_uniform(rng, n, lo, hi):
    return (10.0 ** rng.uniform(np.log10(lo), np.log10(hi), n)).astype(np.float32)


def _sign(rng, n):
    return np.where(rng.random(n) < 0.5, -1.0, 1.0).astype(np.float32)


def build_table(specs, rng):
    """One ``Case`` per spec.  Every array is a view into its own allocation (4 floats of slack to reach the offset)."""
    cases = []
    for s in specs:
        n = s.n
        if s.mode == SELECTIVE:
            assert s.row_width > 0 and n % s.row_width == 0, (n, s.row_width)
        g = _sign(rng, n) * _log_uniform(rng, n, 1e-3, 1.0)
        zeros = rng.choice(n, n // 20, replace=False) if n else np.zeros(0, np.int64)
        g[zeros] = 0.0
        values = {"p": _sign(rng, n) * rng.uniform(0.1, 2.0, n).astype(np.float32), "g": g,
                  "m": _sign(rng, n) * _log_uniform(rng, n, 1e-3, 1.0), "v": _log_uniform(rng, n, 1e-6, 1.0)}
        if s.zero_v:
            assert zeros.size > 0, "zero_v needs a tensor of at least 20 elements"
            values["v"][zeros] = 0.0
        padded = {}
        for name, off in zip(ARRAYS, s.offsets):
            store = np.empty(PAD + n + PAD + 4, np.float32)
            k = slice_start(store.ctypes.data, off)
            view = store[k:k + PAD + n + PAD]
            view[:] = SENTINEL
            view[PAD:PAD + n] = values[name]
            padded[name] = view
        vis = None
        if s.mode == SELECTIVE:
            if s.vis == "alt":
                vis = (np.arange(s.rows) % 2 == 0).astype(np.uint8)
            else:
                vis = (rng.random(s.rows) < s.vis).astype(np.uint8)
        cases.append(Case(s, padded, vis))
    return cases


def dense_constants(spec):
    """(1 - b1, b2, 1 - b2, -step_size, bc2_sqrt, eps) as _wrapper.adam_desc rounds them: computed in double as
    torch.optim.adam._single_tensor_adam does, each rounded once to float32."""
    b1, b2 = spec.betas
    return (f32(1 - b1), f32(b2), f32(1 - b2), -f32(spec.lr / (1 - b1 ** spec.step)), f32((1 - b2 ** spec.step) ** 0.5), f32(spec.eps))


def selective_constants(spec):
    return f32(spec.lr), f32(spec.betas[0]), f32(spec.betas[1]), f32(spec.eps)


def restate_f32(case, dense_c=None, selective_c=None):
    """The float32 restatement of one case; the constants default to the ones the wrapper would put into the descriptor."""
    s = case.spec
    p, g, m, v = (case.data(k).copy() for k in ARRAYS)
    if s.mode == SELECTIVE:
        return selective_f32(p, g, m, v, case.vis, s.row_width, selective_constants(s) if selective_c is None else selective_c)
    return dense_f32(p, g, m, v, dense_constants(s) if dense_c is None else dense_c)


def oracle_f64(case):
    s = case.spec
    p, g, m, v = (case.data(k) for k in ARRAYS)
    if s.mode == SELECTIVE:
        return selective_f64(p, g, m, v, case.vis, s.row_width, s.lr, s.betas[0], s.betas[1], s.eps)
    return dense_f64(p, g, m, v, s.lr, s.betas[0], s.betas[1], s.eps, s.step)


# ---------------------------------------------------------------------------
# the named tables
# ---------------------------------------------------------------------------
CHUNK = 4 * BLOCK
EDGE_SIZES = (1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 1027, 3 * CHUNK - 1, 3 * CHUNK, 3 * CHUNK + 1, 3 * CHUNK + 3)
MISMATCHED_SIZES = (3, 5, 1025, 3 * CHUNK + 1)
MISMATCHED_OFFSETS = ((0, 4, 8, 12), (4, 4, 4, 0), (12, 0, 12, 12), (8, 8, 0, 8))
SELECTIVE_WIDTHS = (1, 2, 3, 4, 5, 7, 45, 48, 1021)
SELECTIVE_VIS = (0.0, 0.25, 1.0, "alt")
BETAS = ((0.9, 0.999), (0.5, 0.999), (0.3, 0.9), (0.0, 0.5))
BETAS_STEPS = (1, 2, 1000)
BETAS_EPS = (1e-15, 1e-8)
SPLIT_COUNTS = (15, 16, 17, 31, 32, 33, 40)
MANY_CHUNKS = (40, 70_000)  # tensors, floats each: 69 chunks apiece
# The split cuts MANY_CHUNKS into launches of 16, 16 and 8 tensors, 1 104 chunks at the most: 2 760 chunks exceed the grid cap of
# an MI355X (256 CUs x 8 blocks = 2 048) only in total.  16 tensors of 137 chunks (2 192) exceed it within ONE launch, where a
# block's second chunk lies 14 or 15 tensors behind its first.
MANY_CHUNKS_ONE_LAUNCH = (TABLE_MAX, 140_000)
_LRS = (1.6e-4, 1e-3, 5e-3, 2e-2, 2.5e-3, 1.25e-4, 7e-4)


def head_offsets(head):
    """All four arrays ``head`` floats ahead of a 16-byte boundary."""
    return ((16 - 4 * head) % 16,) * 4


def _hyper(i):
    """Hyper-parameters that differ from one descriptor to the next."""
    return dict(lr=_LRS[i % len(_LRS)] * (1 + i / 64), betas=BETAS[i % len(BETAS)], eps=BETAS_EPS[(i // 2) % 2], step=1 + 3 * i)


def _width_for(n):
    return next(w for w in (2, 3, 5, 7, 1) if n % w == 0)


def _flag_zero_v(specs):
    """One tensor of the table (the first of at least 1000 floats) gets v = 0 where g = 0, with eps = 1e-8."""
    i = next(i for i, s in enumerate(specs) if s.n >= 1000)
    specs[i] = dataclasses.replace(specs[i], zero_v=True, eps=1e-8)
    return specs


def edge_table(head):
    """EDGE_SIZES in dense mode, all four arrays ``head`` floats ahead of a 16-byte boundary."""
    return _flag_zero_v([Spec(DENSE, n, head_offsets(head), **_hyper(i)) for i, n in enumerate(EDGE_SIZES)])


def edge_table_mismatched():
    return _flag_zero_v([Spec(DENSE, n, off, **_hyper(4 * i + j)) for i, n in enumerate(MISMATCHED_SIZES)
                         for j, off in enumerate(MISMATCHED_OFFSETS)])


def selective_rows(width):
    return 5 if width == 1021 else 4503 // width  # n in 3000 .. 6000


def selective_table(offsets):
    """SELECTIVE_WIDTHS x SELECTIVE_VIS; ``offsets``: a head (int, equal offsets) or "mismatched"."""
    specs = []
    for i, w in enumerate(SELECTIVE_WIDTHS):
        for j, vis in enumerate(SELECTIVE_VIS):
            k = len(SELECTIVE_VIS) * i + j
            off = MISMATCHED_OFFSETS[k % len(MISMATCHED_OFFSETS)] if offsets == "mismatched" else head_offsets(offsets)
            specs.append(Spec(SELECTIVE, selective_rows(w) * w, off, row_width=w, vis=vis, **_hyper(k)))
    i = next(i for i, s in enumerate(specs) if s.vis == "alt")
    specs[i] = dataclasses.replace(specs[i], zero_v=True, eps=1e-8)
    return specs


def betas_table():
    """BETAS x BETAS_STEPS x BETAS_EPS, dense, 1027 floats each, the heads cycling.  The learning rates are small (step_size <=
    2e-3) so that one float32 rounding of exp_avg, divided by the smallest denom, stays inside the bounds of the comparison with
    torch.optim.Adam, whose kernels may contract a multiply-add that this kernel rounds twice."""
    specs = []
    for betas in BETAS:
        for step in BETAS_STEPS:
            for eps in BETAS_EPS:
                k = len(specs)
                specs.append(Spec(DENSE, 1027, head_offsets(k % 4), lr=1e-4 * (1 + k / 24), betas=betas, eps=eps, step=step))
    specs[1] = dataclasses.replace(specs[1], zero_v=True)  # (eps = 1e-8)
    return specs


def split_table(count, with_empty=False):
    """``count`` descriptors, modes alternating, sizes cycling through EDGE_SIZES, every descriptor with its own constants.
    with_empty: the descriptors at positions 0, 15, 16 and last have n = 0 (the GPU test gives them null pointers)."""
    specs = []
    for i in range(count):
        n = EDGE_SIZES[i % len(EDGE_SIZES)]
        off = MISMATCHED_OFFSETS[i % 4] if i % 5 == 4 else head_offsets(i % 4)
        if i % 2:
            specs.append(Spec(SELECTIVE, n, off, row_width=_width_for(n), vis=("alt", 1.0, 0.25, "alt")[(i // 2) % 4], **_hyper(i)))
        else:
            specs.append(Spec(DENSE, n, off, **_hyper(i)))
    _flag_zero_v(specs)
    if with_empty:
        for i in {0, 15, 16, count - 1}:
            if i < count:
                specs[i] = dataclasses.replace(specs[i], n=0, zero_v=False)
    return specs


def many_chunks_table(one_launch=False):
    count, n = MANY_CHUNKS_ONE_LAUNCH if one_launch else MANY_CHUNKS
    return _flag_zero_v([Spec(DENSE, n, head_offsets(i % 4), **_hyper(i)) for i in range(count)])


def chunks_of(spec):
    """The kernel's chunk count of one descriptor (optim.hip: head, quads, the c == 0 -> 1 rule)."""
    if spec.n == 0:
        return 0
    head = (16 - spec.offsets[0]) % 16 // 4 if len(set(spec.offsets)) == 1 else 0
    head = min(head, spec.n)
    quads = (spec.n - head + 3) // 4
    return max(1, -(-quads // BLOCK))


def named_tables():
    """(name, specs) of every table the GPU test runs."""
    out = [(f"edge head {h}", edge_table(h)) for h in range(4)] + [("edge mismatched", edge_table_mismatched())]
    out += [(f"selective {'head ' + str(o) if o != 'mismatched' else o}", selective_table(o)) for o in (0, 3, "mismatched")]
    out.append(("betas", betas_table()))
    out += [(f"split {c}{' with empty' if e else ''}", split_table(c, e)) for c in SPLIT_COUNTS for e in (False, True)]
    out.append(("many chunks", many_chunks_table()))
    out.append(("many chunks in one launch", many_chunks_table(True)))
    return out


def table_rng(name):
    """A generator of its own for every named table: the CPU and the GPU tests see the same values."""
    return np.random.default_rng([20240607] + [ord(ch) for ch in name])
