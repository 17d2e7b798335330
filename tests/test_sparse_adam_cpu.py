"""CPU: the numpy restatement of gs_sparse_adam_multi (tests/sparse_adam_cases.py) against torch.optim.SparseAdam bit for bit
on the inputs where torch's own summation order of duplicates cannot matter, its distance from the float64 oracle on every named
call, the checks of optimizers.SparseAdam that precede any launch, sparsify_grads, and the exports.  No kernel runs here."""
import ctypes

import numpy as np
import pytest
import torch

import adam_cases as AC
import sparse_adam_cases as SC

LR, EPS, BETAS = 1.6e-4, 1e-15, (0.9, 0.999)  # the trainer's means optimizer
ROWS = 600


def _step_ids(dup, rng):
    """(ids, exact): fresh indices of one step.  exact: the values have to be multiples of 1/1024 (sums of them are exact)."""
    if dup == "none":
        return rng.permutation(ROWS)[:200].astype(np.int64), False
    if dup == "twice":
        return rng.permutation(np.repeat(rng.permutation(ROWS)[:150], 2)).astype(np.int64), False
    if dup == "four exact":
        return rng.permutation(np.repeat(rng.permutation(ROWS)[:60], 4)).astype(np.int64), True
    assert dup == "300 exact"
    others = rng.permutation(ROWS - 1)[:50] + 1
    return rng.permutation(np.concatenate([np.zeros(300, np.int64), others])).astype(np.int64), True


@pytest.mark.parametrize("dup", ["none", "twice", "four exact", "300 exact"])
@pytest.mark.parametrize("width", SC.ROW_WIDTHS)
def test_restatement_equals_torch_sparse_adam_bit_for_bit(width, dup):
    """5 steps of torch.optim.SparseAdam on CPU tensors, fresh indices per step, against sparse_f32 carried along: parameters and
    both moments identical in every bit after every step."""
    rng = np.random.default_rng([7, width, len(dup)])
    shape = (ROWS,) if width == 1 else (ROWS, width)
    p0 = (AC._sign(rng, ROWS * width) * rng.uniform(0.1, 2.0, ROWS * width).astype(np.float32)).reshape(ROWS, width)
    param = torch.nn.Parameter(torch.from_numpy(p0.reshape(shape).copy()))
    opt = torch.optim.SparseAdam([param], lr=LR, betas=BETAS, eps=EPS)
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for step in range(1, 6):
        ids, exact = _step_ids(dup, rng)
        if exact:
            values = (rng.integers(-512, 513, (ids.size, width)) / 1024.0).astype(np.float32)
        else:
            values = (AC._sign(rng, ids.size * width) * AC._log_uniform(rng, ids.size * width, 1e-3, 1.0)).reshape(-1, width)
        param.grad = torch.sparse_coo_tensor(torch.from_numpy(ids)[None], torch.from_numpy(values.reshape((-1,) + shape[1:]).copy()), shape)
        opt.step()
        p, m, v = SC.sparse_f32(p, m, v, values, ids, SC.constants(LR, BETAS[0], BETAS[1], EPS, step))
        st = opt.state[param]
        assert st["step"] == step
        for name, mine, theirs in (("p", p, param.detach()), ("exp_avg", m, st["exp_avg"]), ("exp_avg_sq", v, st["exp_avg_sq"])):
            differ = int((AC.bits(mine) != AC.bits(theirs.numpy().reshape(ROWS, width))).sum())
            assert differ == 0, f"width {width}, {dup}, step {step}: {differ} elements of {name} differ in bits"


def test_restatement_against_float64_on_every_named_call(capsys):
    """The distance the GPU test's bound is built from, largest over each call's descriptors; rows without an index keep their
    bits in the restatement and the oracle alike."""
    lines = []
    for call in SC.named_calls():
        case = SC.build_call(call, SC.call_rng(call.name))
        worst = dict.fromkeys(SC.OUT, 0.0)
        for i in range(len(call.descs)):
            got, ref = case.restate_f32(i), case.oracle_f64(i)
            hidden = ~case.touched(i)
            for k, x, r in zip(SC.OUT, got, ref):
                assert np.array_equal(AC.bits(x.ravel())[hidden], AC.bits(case.data(i, k).ravel())[hidden]), (call.name, i, k)
                assert np.array_equal(r.ravel()[hidden], case.data(i, k).ravel()[hidden].astype(np.float64)), (call.name, i, k)
                e = AC.rel_err(x, r)
                assert np.isfinite(e) and e < 0.1, (call.name, i, k, e)
                worst[k] = max(worst[k], e)
            if call.nnz:
                assert not np.array_equal(got[0], case.data(i, "p")), (call.name, i)
        lines.append(f"    {call.name:36s} " + "   ".join(f"{worst[k]:.2e}" for k in SC.OUT))
    with capsys.disabled():
        print("\n    call                                 p          exp_avg    exp_avg_sq\n" + "\n".join(lines))


def test_named_calls_cover_the_patterns():
    calls = SC.named_calls()
    assert len({c.name for c in calls}) == len(calls)
    assert {(c.rows, c.nnz) for c in calls} >= {(r, n) for r in SC.ROWS for n in SC.NNZ}
    assert {c.pattern for c in calls} == set(SC.PATTERNS) | {"run of 300", "runs at both ends"}
    assert {d.row_width for c in calls for d in c.descs} == set(SC.ROW_WIDTHS)
    assert {d.values_offset for c in calls for d in c.descs if d.row_width == 45} == {0, 4, 8, 12}
    assert max(len(c.descs) for c in calls) == SC.TABLE_MAX + 1
    rng = np.random.default_rng(3)
    for pat in ("every id twice", "mixed runs", "shuffled unique", "random"):
        ids = SC.make_ids(pat, 1000, 257, rng)
        assert ids.min() == 0 and ids.max() == 999, pat
    _, _, lengths = SC.runs_of(SC.make_ids("mixed runs", 1000, 1000, rng))
    assert set(lengths) == {1, 2, 3, 4}
    case = SC.build_call(SC.special_calls()[1], rng)
    assert (case.sorted_ids[:3] == 0).all() and (case.sorted_ids[-3:] == 999).all()  # runs from position 0 and up to nnz - 1
    _, _, lengths = SC.runs_of(SC.ids_run_of_300(rng))
    assert lengths.max() == 300


def _sparse_param(dtype=torch.float32, sparse_dim=1):
    p = torch.nn.Parameter(torch.ones(6, 3, dtype=dtype))
    if sparse_dim == 1:
        p.grad = torch.sparse_coo_tensor(torch.tensor([[1, 4]]), torch.ones(2, 3, dtype=dtype), (6, 3))
    else:
        p.grad = torch.sparse_coo_tensor(torch.tensor([[1, 4], [0, 2]]), torch.ones(2, dtype=dtype), (6, 3))
    return p


@pytest.mark.parametrize("way,exc,match", [
    ("cpu", RuntimeError, "is on cpu"),
    ("dense", RuntimeError, "SparseAdam does not support dense gradients, please consider Adam instead"),
    ("sparse_dim 2", RuntimeError, "2 sparse dimensions"),
    ("float64", RuntimeError, "float64"),
    ("maximize", ValueError, "maximize"),
    ("tensor lr", ValueError, "tensor lr"),
])
@pytest.mark.parametrize("through", ["step", "step_all"])
def test_validation_precedes_any_mutation(way, exc, match, through):
    """Nothing is launched and nothing mutated: the state stays empty, a seeded state keeps its step and bits, and the other
    optimizer of a step_all call is not advanced either."""
    from gscodec_studio_amd.optimizers import SparseAdam, step_all

    p = _sparse_param(torch.float64 if way == "float64" else torch.float32, 2 if way == "sparse_dim 2" else 1)
    if way == "dense":
        p.grad = torch.ones(6, 3)
    if way == "tensor lr":
        with pytest.raises(ValueError, match=match):
            SparseAdam([p], lr=torch.tensor(1e-3))
        opt = torch.optim.SparseAdam([p], lr=torch.tensor(1e-3))  # (torch's own class, as step_all also takes it)
        through = "step_all"
    else:
        opt = SparseAdam([{"params": [p], "name": "sh0"}], lr=1e-3)
        if way == "maximize":  # refused by the constructor, and by the step when a group is switched later
            with pytest.raises(ValueError, match=match):
                SparseAdam([p], lr=1e-3, maximize=True)
            opt.param_groups[0]["maximize"] = True
    seeded = way in ("cpu", "dense")
    if seeded:
        opt.state[p] = {"step": 3, "exp_avg": torch.full_like(p, 0.25), "exp_avg_sq": torch.full_like(p, 0.5)}
    before = p.detach().clone()
    q = _sparse_param()
    front = SparseAdam([q], lr=1e-3)
    with pytest.raises(exc, match=match):
        if through == "step":
            opt.step()
        else:
            step_all([opt, front])
    assert torch.equal(p.detach(), before) and p.grad is not None
    assert len(front.state) == 0 and q.grad is not None
    if seeded:
        st = opt.state[p]
        assert st["step"] == 3 and bool((st["exp_avg"] == 0.25).all()) and bool((st["exp_avg_sq"] == 0.5).all())
    else:
        assert len(opt.state) == 0


def test_state_dict_layout_is_torchs():
    from gscodec_studio_amd.optimizers import SparseAdam

    p = _sparse_param()
    ours, theirs = SparseAdam([p], lr=2e-3, betas=(0.8, 0.99), eps=1e-12), torch.optim.SparseAdam([_sparse_param()], lr=1e-3)
    ours.state[p] = {"step": 4, "exp_avg": torch.full_like(p, 0.25), "exp_avg_sq": torch.full_like(p, 0.5)}
    theirs.load_state_dict(ours.state_dict())
    back = SparseAdam([_sparse_param()], lr=1e-3)
    back.load_state_dict(theirs.state_dict())
    (st,) = back.state.values()
    assert st["step"] == 4 and isinstance(st["step"], int) and bool((st["exp_avg"] == 0.25).all())
    assert back.param_groups[0]["lr"] == 2e-3 and back.param_groups[0]["betas"] == (0.8, 0.99) and back.param_groups[0]["maximize"] is False
    assert issubclass(SparseAdam, torch.optim.SparseAdam)


def test_descriptor_scalars_equal_torch_formula():
    from gscodec_studio_amd.optimizers import sparse as S

    lr, beta1, beta2, eps = 1.6e-4 * 0.7, 0.9, 0.999, 1e-15
    t = torch.zeros(8, 2)
    for step in (1, 2, 1000):
        d = S.sparse_adam_desc(t, t, t, t, 2, lr, beta1, beta2, eps, step)
        w1, w2, s, e = SC.constants(lr, beta1, beta2, eps, step)
        assert (d.one_minus_beta1, d.one_minus_beta2, d.neg_step_size, d.eps, d.row_width) == (float(w1), float(w2), float(s), float(e), 2)
        import math

        assert d.neg_step_size == float(np.float32(-(lr * math.sqrt(1 - beta2 ** step) / (1 - beta1 ** step))))


def test_sparse_adam_multi_is_declared_exported_and_guarded():
    from gscodec_studio_amd import _backend as B
    from gscodec_studio_amd.optimizers import sparse as S

    protos = B.prototypes()
    for name in ("gs_sparse_adam_multi", "gs_sparse_adam_desc_layout"):
        assert name in protos and hasattr(B.lib(), name), name
    cls = S.sparse_adam_desc_class()
    assert cls is B.struct("gs_sparse_adam_desc") and [f[0] for f in cls._fields_] == list(S._DESC_FIELDS)
    assert int(B.query("gs_sparse_adam_desc_layout", None, 0)) == 1 + len(S._DESC_FIELDS)
    with pytest.raises(ImportError, match="struct layout"):  # a guard that names the fields in another order is refused
        B.guarded_struct("gs_sparse_adam_desc", "gs_sparse_adam_desc_layout", S._DESC_FIELDS[::-1])
    # the guards of the C entry precede the launch (no device needed to reach them)
    d = cls()
    table = (cls * 1)(d)
    ids = (ctypes.c_int64 * 4)(0, 1, 2, 3)
    addr = ctypes.addressof(ids)
    with pytest.raises(RuntimeError, match="descriptor 0: null pointer"):
        B.call("gs_sparse_adam_multi", 1, ctypes.addressof(table), 4, addr, None, 8, None)
    d.param = d.exp_avg = d.exp_avg_sq = d.values = addr  # (never dereferenced: the host refuses the call)
    for width, nnz, rows, match in ((0, 4, 8, "row_width"), (3, 4, 1 << 31, "rows \\* row_width"), (1 << 30, 4, 2, "nnz \\* row_width")):
        d.row_width = width
        table = (cls * 1)(d)
        with pytest.raises(RuntimeError, match=match):
            B.call("gs_sparse_adam_multi", 1, ctypes.addressof(table), nnz, addr, None, rows, None)
    d.row_width = 3
    d.values = addr + 2
    table = (cls * 1)(d)
    with pytest.raises(RuntimeError, match="4-byte aligned"):
        B.call("gs_sparse_adam_multi", 1, ctypes.addressof(table), 4, addr, None, 8, None)
    with pytest.raises(RuntimeError, match="nnz must be < 2\\^31"):
        B.call("gs_sparse_adam_multi", 1, ctypes.addressof(table), 1 << 31, addr, None, 8, None)
    B.call("gs_sparse_adam_multi", 1, ctypes.addressof(table), 0, None, None, 8, None)  # nnz == 0: nothing is launched


def test_sparsify_grads_is_the_trainers_loop():
    from gscodec_studio_amd.optimizers import sparsify_grads

    g = torch.Generator().manual_seed(1)
    for coalesced, ids in ((True, torch.tensor([0, 2, 5, 6])), (False, torch.tensor([5, 2, 5, 0, 6]))):
        splats = torch.nn.ParameterDict({"means": torch.nn.Parameter(torch.rand(8, 3, generator=g)),
                                         "opacities": torch.nn.Parameter(torch.rand(8, generator=g)),
                                         "shN": torch.nn.Parameter(torch.rand(8, 15, 3, generator=g)),
                                         "quats": torch.nn.Parameter(torch.rand(8, 4, generator=g)),
                                         "scales": torch.nn.Parameter(torch.rand(8, 3, generator=g))})
        dense = {k: torch.rand(p.shape, generator=g) for k, p in splats.items()}
        for k in ("means", "opacities", "shN"):
            splats[k].grad = dense[k].clone()
        already = torch.sparse_coo_tensor(torch.tensor([[1]]), torch.ones(1, 4), (8, 4))
        splats["quats"].grad = already
        sparsify_grads(splats, ids, coalesced)
        assert splats["scales"].grad is None and splats["quats"].grad is already
        for k in ("means", "opacities", "shN"):
            got = splats[k].grad
            want = torch.sparse_coo_tensor(indices=ids[None], values=dense[k][ids], size=splats[k].size(), is_coalesced=coalesced)
            assert got.is_sparse and got.shape == splats[k].shape and got.is_coalesced() == want.is_coalesced() == coalesced
            assert got._indices().data_ptr() == ids.data_ptr() and got._indices().shape == (1, ids.numel())
            assert torch.equal(got._values(), want._values()) and torch.equal(got.to_dense(), want.to_dense())
        # an iterable of parameters works as the dict does
        splats["means"].grad = dense["means"].clone()
        sparsify_grads([splats["means"]], ids, coalesced)
        assert splats["means"].grad._indices().data_ptr() == ids.data_ptr()


def test_exports():
    import gscodec_studio_amd.optimizers as O

    assert {"SparseAdam", "sparsify_grads", "step_all", "Adam", "SelectiveAdam", "visibility_mask"} <= set(O.__all__)
    assert O.SparseAdam is O.sparse.SparseAdam and callable(O.sparsify_grads)
