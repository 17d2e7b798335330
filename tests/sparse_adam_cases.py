"""Reference arithmetic, the table builder and the named cases shared by tests/test_sparse_adam_cpu.py and
tests/test_gpu_sparse_adam.py (gs_sparse_adam_multi, csrc/optim.hip).  Plain numpy: no fixtures, no pytest hooks.

* ``sparse_f32``: the kernel's update restated in numpy float32, one rounding per operation, from the float constants the
  descriptor carries; the duplicates of an id are summed in ascending position in ``values``, starting from the first value
  (the order a stable sort on (id, position) gives the kernel).  ``sparse_f64``: the same update in float64 from the double
  hyper-parameters (torch.optim.SparseAdam's formula: step_size = lr * sqrt(1 - beta2^step) / (1 - beta1^step), eps outside
  the bias correction).  Rows whose id does not occur keep their old values in both.
* ``build_call(call, rng)``: host arrays for one ``Call`` (one index list, several descriptors); p, exp_avg, exp_avg_sq and
  values of every descriptor sit between 8 sentinel floats (adam_cases.SENTINEL), values at the requested byte offset mod 16.
* The named cases: ``named_calls()`` -- ROW_WIDTHS x ROWS x NNZ with every index pattern that fits, and the special calls
  (a run of 300, runs at both ends of the sorted list, 17 descriptors).

Value ranges as in adam_cases: |g| in [1e-3, 1] with n // 20 entries exactly 0, |m| in [1e-3, 1], v in [1e-6, 1] (log-uniform),
|p| in [0.1, 2].

The GPU test computes the distance of the restatement from the float64 oracle per descriptor and holds the kernel to twice that
plus one float32 ulp (adam_cases' rule); test_sparse_adam_cpu.py prints the distances per named call.
"""
import dataclasses
from typing import Optional, Tuple

import numpy as np

import adam_cases as AC

f32 = np.float32
PAD, SENTINEL, SENTINEL_BITS, ULP = AC.PAD, AC.SENTINEL, AC.SENTINEL_BITS, AC.ULP
TABLE_MAX = AC.TABLE_MAX  # GS_ADAM_MULTI_MAX: the sparse call splits at the same count
OUT = ("p", "m", "v")

ROW_WIDTHS = (1, 3, 4, 45)
ROWS = (1, 7, 1000)
NNZ = (0, 1, 255, 256, 257, 1000)
VALUE_OFFSETS = (0, 4, 8, 12)
PATTERNS = ("sorted unique", "shuffled unique", "every id twice", "mixed runs", "random")


# ---------------------------------------------------------------------------
# the update, float32 as the kernel rounds it and float64
# ---------------------------------------------------------------------------
def runs_of(ids):
    """(order, starts, lengths): the stable (id, position) order of ``ids`` and its runs of equal ids."""
    ids = np.asarray(ids, np.int64)
    order = np.argsort(ids, kind="stable")
    s = ids[order]
    starts = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]])) if ids.size else np.zeros(0, np.int64)
    lengths = np.diff(np.concatenate([starts, [ids.size]]))
    return order, starts, lengths


def sum_duplicates(values, ids, dtype):
    """(unique ids ascending, their summed value rows): every run added up in ascending position, one rounding of ``dtype`` per
    addition, starting from the run's first value."""
    values = np.asarray(values)
    order, starts, lengths = runs_of(ids)
    uniq = np.asarray(ids, np.int64)[order[starts]] if starts.size else np.zeros(0, np.int64)
    g = values[order[starts]].astype(dtype)
    for r in range(1, int(lengths.max()) if lengths.size else 0):
        has = lengths > r
        g[has] = g[has] + values[order[starts[has] + r]].astype(dtype)
    assert g.dtype == dtype
    return uniq, g


def sparse_f32(p, m, v, values, ids, c):
    """The step of optim.hip's SparseAdam comment.  p, m, v: float32 [rows, width]; values float32 [nnz, width]; ids [nnz];
    c = (one_minus_beta1, one_minus_beta2, neg_step_size, eps), the float32 values of the descriptor.  Returns new (p, m, v)."""
    for a in (p, m, v, values):
        assert a.dtype == np.float32 and a.ndim == 2, (a.dtype, a.shape)
    w1, w2, s, eps = (f32(x) for x in c)
    uniq, g = sum_duplicates(values, ids, np.float32)
    p1, m1, v1 = p.copy(), m.copy(), v.copy()
    mo, vo = m[uniq], v[uniq]
    d1 = (g - mo) * w1
    d2 = (g * g - vo) * w2
    m1[uniq] = mo + d1
    v1[uniq] = vo + d2
    upd = s * ((d1 + mo) / (np.sqrt(d2 + vo) + eps))
    p1[uniq] = p[uniq] + upd
    for a in (p1, m1, v1, upd, d1, d2):
        assert a.dtype == np.float32
    return p1, m1, v1


def sparse_f64(p, m, v, values, ids, lr, beta1, beta2, eps, step):
    p, m, v, values = (np.asarray(a, np.float64) for a in (p, m, v, values))
    uniq, g = sum_duplicates(values, ids, np.float64)
    p1, m1, v1 = p.copy(), m.copy(), v.copy()
    m1[uniq] = beta1 * m[uniq] + (1.0 - beta1) * g
    v1[uniq] = beta2 * v[uniq] + (1.0 - beta2) * g * g
    step_size = lr * np.sqrt(1.0 - beta2 ** step) / (1.0 - beta1 ** step)
    p1[uniq] = p[uniq] - step_size * m1[uniq] / (np.sqrt(v1[uniq]) + eps)
    return p1, m1, v1


def constants(lr, beta1, beta2, eps, step):
    """(1 - b1, 1 - b2, -step_size, eps) as optimizers.sparse rounds them: computed in double as
    torch.optim._functional.sparse_adam does, each rounded once to float32."""
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    return f32(1 - beta1), f32(1 - beta2), f32(-(lr * float(np.sqrt(bc2)) / bc1)), f32(eps)


# ---------------------------------------------------------------------------
# index patterns
# ---------------------------------------------------------------------------
def _distinct(rng, rows, count):
    """``count`` distinct ids of [0, rows), 0 and rows - 1 among them where count >= 2 (or rows == 1)."""
    assert count <= rows, (count, rows)
    if count == 0:
        return np.zeros(0, np.int64)
    if count == 1:
        return np.array([0 if rows == 1 else rng.integers(rows)], np.int64)
    inner = rng.choice(np.arange(1, rows - 1), count - 2, replace=False) if count > 2 else np.zeros(0, np.int64)
    return np.concatenate([[0, rows - 1], inner]).astype(np.int64)


def _run_lengths(pattern, nnz):
    if pattern == "every id twice":
        return [2] * (nnz // 2) + [1] * (nnz % 2)
    out = []
    while sum(out) < nnz:  # mixed runs: 1, 2, 3, 4, 1, ...
        out.append(min(len(out) % 4 + 1, nnz - sum(out)))
    return out


def pattern_fits(pattern, rows, nnz):
    if nnz == 0:
        return pattern == "sorted unique"
    if pattern in ("sorted unique", "shuffled unique"):
        return nnz <= rows
    if pattern == "random":
        return True
    return nnz >= 2 and len(_run_lengths(pattern, nnz)) <= rows


def make_ids(pattern, rows, nnz, rng):
    """int64 [nnz] in [0, rows).  Everything but "sorted unique" is shuffled in position."""
    assert pattern_fits(pattern, rows, nnz), (pattern, rows, nnz)
    if pattern == "sorted unique":
        return np.sort(_distinct(rng, rows, nnz))
    if pattern == "shuffled unique":
        return rng.permutation(_distinct(rng, rows, nnz))
    if pattern == "random":
        ids = rng.integers(0, rows, nnz).astype(np.int64)
        if nnz >= 2:
            ids[rng.choice(nnz, 2, replace=False)] = (0, rows - 1)
        return ids
    lengths = _run_lengths(pattern, nnz)
    return rng.permutation(np.repeat(rng.permutation(_distinct(rng, rows, len(lengths))), lengths))


def ids_run_of_300(rng, rows=1000, nnz=1000):
    """One id 300 times, the others once: at row_width 1 the run crosses a 256-lane workgroup wherever it starts."""
    others = rng.choice(np.delete(np.arange(rows), 500), nnz - 300, replace=False)
    return rng.permutation(np.concatenate([np.full(300, 500), others]).astype(np.int64))


def ids_runs_at_both_ends(rng, rows, nnz):
    """Id 0 three times (its run starts at sorted position 0), id rows - 1 three times (its run ends at nnz - 1), the rest once."""
    others = rng.choice(np.arange(1, rows - 1), nnz - 6, replace=False)
    return rng.permutation(np.concatenate([[0] * 3, [rows - 1] * 3, others]).astype(np.int64))


# ---------------------------------------------------------------------------
# calls and the table builder
# ---------------------------------------------------------------------------
_LRS = (1.6e-4, 1e-3, 5e-3, 2e-2, 2.5e-3, 1.25e-4, 7e-4)
_BETAS = ((0.9, 0.999), (0.5, 0.999), (0.3, 0.9), (0.0, 0.5))


@dataclasses.dataclass(frozen=True)
class Desc:
    row_width: int
    values_offset: int = 0        # byte offset mod 16 of the values' base pointer
    lr: float = 1.6e-4
    betas: Tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-15
    step: int = 1                 # the advanced step counter


@dataclasses.dataclass(frozen=True)
class Call:
    name: str
    rows: int
    nnz: int
    pattern: str                  # one of PATTERNS, "run of 300" or "runs at both ends"
    descs: Tuple[Desc, ...]


@dataclasses.dataclass
class Case:
    call: Call
    ids: np.ndarray               # int64 [nnz], as the gradient carries them
    sorted_ids: np.ndarray        # int64 [nnz]
    perm: Optional[np.ndarray]    # int32 [nnz]; None for "sorted unique" (identity)
    padded: list                  # per descriptor: name -> float32 [PAD + n + PAD]; "g" at the descriptor's offset

    def data(self, i, name):
        d = self.call.descs[i]
        n = (self.call.nnz if name == "g" else self.call.rows) * d.row_width
        return self.padded[i][name][PAD:PAD + n].reshape(-1, d.row_width)

    def constants(self, i):
        d = self.call.descs[i]
        return constants(d.lr, d.betas[0], d.betas[1], d.eps, d.step)

    def restate_f32(self, i, c=None):
        p, m, v, g = (self.data(i, k).copy() for k in ("p", "m", "v", "g"))
        return sparse_f32(p, m, v, g, self.ids, self.constants(i) if c is None else c)

    def oracle_f64(self, i):
        d = self.call.descs[i]
        p, m, v, g = (self.data(i, k) for k in ("p", "m", "v", "g"))
        return sparse_f64(p, m, v, g, self.ids, d.lr, d.betas[0], d.betas[1], d.eps, d.step)

    def touched(self, i):
        """bool [rows * width]: the elements of the rows that have an index."""
        rows = np.zeros(self.call.rows, bool)
        rows[self.ids] = True
        return np.repeat(rows, self.call.descs[i].row_width)


def _padded(values, offset):
    store = np.empty(PAD + values.size + PAD + 4, np.float32)
    k = AC.slice_start(store.ctypes.data, offset)
    view = store[k:k + PAD + values.size + PAD]
    view[:] = SENTINEL
    view[PAD:PAD + values.size] = values
    return view


def build_call(call, rng):
    if call.pattern == "run of 300":
        ids = ids_run_of_300(rng, call.rows, call.nnz)
    elif call.pattern == "runs at both ends":
        ids = ids_runs_at_both_ends(rng, call.rows, call.nnz)
    else:
        ids = make_ids(call.pattern, call.rows, call.nnz, rng)
    assert ids.shape == (call.nnz,) and (ids.size == 0 or (ids.min() >= 0 and ids.max() < call.rows))
    order = np.argsort(ids, kind="stable")
    perm = None if call.pattern == "sorted unique" else order.astype(np.int32)
    padded = []
    for d in call.descs:
        n, ng = call.rows * d.row_width, call.nnz * d.row_width
        g = AC._sign(rng, ng) * AC._log_uniform(rng, ng, 1e-3, 1.0)
        if ng:
            g[rng.choice(ng, ng // 20, replace=False)] = 0.0
        padded.append({"p": _padded(AC._sign(rng, n) * rng.uniform(0.1, 2.0, n).astype(np.float32), 0),
                       "m": _padded(AC._sign(rng, n) * AC._log_uniform(rng, n, 1e-3, 1.0), 0),
                       "v": _padded(AC._log_uniform(rng, n, 1e-6, 1.0), 0),
                       "g": _padded(g, d.values_offset)})
    return Case(call, ids, ids[order], perm, padded)


def _descs(count, shift=0):
    """``count`` descriptors: the widths cycling through ROW_WIDTHS, every one with its own constants and values offset."""
    return tuple(Desc(ROW_WIDTHS[i % 4], VALUE_OFFSETS[(i + i // 4 + shift) % 4], lr=_LRS[(i + shift) % len(_LRS)] * (1 + i / 64),
                      betas=_BETAS[(i + shift) % 4], eps=(1e-15, 1e-8)[(i // 2) % 2], step=1 + 3 * i + shift) for i in range(count))


def grid_calls(rows, nnz):
    """Every pattern that fits (rows, nnz), four descriptors (ROW_WIDTHS) each."""
    return [Call(f"rows {rows} nnz {nnz} {pat}", rows, nnz, pat, _descs(4, shift=k))
            for k, pat in enumerate(PATTERNS) if pattern_fits(pat, rows, nnz)]


def special_calls():
    return [Call("run of 300", 1000, 1000, "run of 300", _descs(4, shift=1)),
            Call("runs at both ends", 1000, 257, "runs at both ends", _descs(4, shift=2)),
            Call("17 descriptors", 1000, 257, "mixed runs", _descs(TABLE_MAX + 1, shift=3))]


def named_calls():
    return [c for rows in ROWS for nnz in NNZ for c in grid_calls(rows, nnz)] + special_calls()


def call_rng(name):
    """A generator of its own for every named call: the CPU and the GPU tests see the same values."""
    return np.random.default_rng([20250611] + [ord(ch) for ch in name])
