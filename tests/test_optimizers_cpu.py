"""gscodec_studio_amd.optimizers without a GPU: the module imports, unsupported Adam settings are refused at construction,
the host-side descriptor scalars equal torch's Adam arithmetic, and the optimizer entry points are part of the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import adam_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_module_imports_and_exports():
    import gscodec_studio_amd
    from gscodec_studio_amd import optimizers
    from gscodec_studio_amd._c_adapter import _C

    for name in ("Adam", "SelectiveAdam", "step_all", "visibility_mask"):
        assert callable(getattr(optimizers, name)), name
    assert issubclass(optimizers.Adam, torch.optim.Adam) and issubclass(optimizers.SelectiveAdam, torch.optim.Adam)
    assert callable(gscodec_studio_amd.selective_adam_update) and callable(_C.selective_adam_update)


@pytest.mark.parametrize("kw", [dict(amsgrad=True), dict(weight_decay=1e-4), dict(maximize=True), dict(capturable=True),
                                dict(differentiable=True), dict(fused=True), dict(lr=torch.tensor(1e-3))])
def test_adam_refuses_unsupported_settings(kw):
    from gscodec_studio_amd.optimizers import Adam

    p = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises((ValueError, RuntimeError)):
        Adam([p], **kw)


def test_adam_refuses_unsupported_group_and_accepts_supported():
    from gscodec_studio_amd.optimizers import Adam

    p, q = torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(4))
    opt = Adam([{"params": [p], "lr": 1e-2, "name": "means"}], eps=1e-15, betas=(0.9, 0.999), foreach=True)
    with pytest.raises(ValueError, match="weight_decay"):
        opt.add_param_group({"params": [q], "weight_decay": 0.1})
    # the state dict has torch.optim.Adam's layout: a plain torch Adam loads it
    torch.optim.Adam([torch.nn.Parameter(torch.zeros(4))], lr=1e-2).load_state_dict(opt.state_dict())


def test_step_needs_gpu_tensors_and_names_the_parameter():
    from gscodec_studio_amd.optimizers import Adam, step_all

    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    opt = Adam([{"params": [p], "name": "opacities"}])
    with pytest.raises(RuntimeError, match="opacities"):
        opt.step()
    assert len(opt.state) == 0  # nothing was initialised or advanced
    with pytest.raises(TypeError):
        step_all([torch.optim.SGD([p], lr=0.1)])


def test_dense_descriptor_scalars_equal_torch_formula():
    """step_size = lr / (1 - b1^step), bc2_sqrt = (1 - b2^step)^0.5 in double (torch.optim.adam._single_tensor_adam),
    1 - b1 / 1 - b2 (the lerp / addcmul weights) -- each rounded once to float in the descriptor."""
    from gscodec_studio_amd import _wrapper as W

    lr, beta1, beta2, eps = 1.6e-4 * 0.7, 0.9, 0.999, 1e-15
    t = torch.zeros(8)
    for step in (1, 2, 1000):
        d = W.adam_desc(W.ADAM_DENSE, t, t, t, t, lr, beta1, beta2, eps, step=float(step))
        f32 = lambda x: float(np.float32(x))  # noqa: E731
        assert d.step_size == f32(lr / (1 - beta1 ** step)), step
        assert d.bias_correction2_sqrt == f32((1 - beta2 ** step) ** 0.5), step
        assert d.one_minus_beta1 == f32(1 - beta1) and d.one_minus_beta2 == f32(1 - beta2)
        assert d.beta2 == f32(beta2) and d.eps == f32(eps) and d.n == 8 and d.mode == W.ADAM_DENSE
    # the selective descriptor carries the reference's float arguments and the row split
    vis = torch.ones(4, dtype=torch.bool)
    d = W.adam_desc(W.ADAM_SELECTIVE, t, t, t, t, 1e-3, 0.9, 0.999, 1e-15, visibility=vis, rows=4, row_width=2, n=8)
    assert (d.rows, d.row_width, d.n, d.mode) == (4, 2, 8, W.ADAM_SELECTIVE) and d.lr == float(np.float32(1e-3))


def test_adam_multi_is_declared_exported_and_mirrored():
    from gscodec_studio_amd import _backend as B
    from gscodec_studio_amd import _wrapper as W

    protos = B.prototypes()
    for name in ("gs_adam_multi", "gs_adam_multi_max", "gs_adam_desc_layout"):
        assert name in protos, name
        assert hasattr(B.lib(), name), name
    hdr = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    assert int(re.search(r"#define GS_ADAM_MULTI_MAX (\d+)", hdr).group(1)) == int(B.query("gs_adam_multi_max"))
    B.check_layouts()  # (gs_adam_desc among them)
    # a bad descriptor is refused before anything is launched (no device needed to reach the check)
    bad = W._AdamDesc()
    bad.n, bad.mode = 16, 7
    table = (W._AdamDesc * 1)(bad)
    with pytest.raises(RuntimeError, match="null pointer|unknown mode"):
        B.call("gs_adam_multi", 1, ctypes.addressof(table), None)


# ---------------------------------------------------------------------------
# tests/adam_cases.py: the references and the table builder that tests/test_gpu_adam_table.py holds the kernel to
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("betas", AC.BETAS)
def test_dense_restatement_matches_torch_cpu_adam(betas):
    """dense_f32, three steps on 1 000 elements, against torch.optim.Adam(foreach=False) on the CPU, with the constants of
    W.adam_dense_scalars and the bounds the GPU tests use for this comparison."""
    from gscodec_studio_amd import _wrapper as W

    lr, eps, n = 1e-3, 1e-15, 1000
    rng = np.random.default_rng(11)
    p0 = (rng.uniform(0.1, 2.0, n) * np.where(rng.random(n) < 0.5, -1, 1)).astype(np.float32)
    p = torch.nn.Parameter(torch.tensor(p0))
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps, foreach=False)
    mine = (p0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32))
    for step in (1, 2, 3):
        g = (rng.standard_normal(n) * 0.3).astype(np.float32)
        g[::20] = 0.0
        p.grad = torch.tensor(g)
        opt.step()
        w1, w2, step_size, bc2_sqrt = W.adam_dense_scalars(lr, betas[0], betas[1], float(step))
        c = tuple(np.float32(x) for x in (w1, betas[1], w2, -step_size, bc2_sqrt, eps))
        mine = AC.dense_f32(mine[0], g, mine[1], mine[2], c)
    st = opt.state[p]
    for got, want, atol in ((mine[0], p.detach(), 1e-7), (mine[1], st["exp_avg"], 1e-6), (mine[2], st["exp_avg_sq"], 1e-9)):
        torch.testing.assert_close(torch.tensor(got), want, rtol=1e-6, atol=atol)


def test_restatement_constants_equal_the_descriptor():
    from gscodec_studio_amd import _wrapper as W

    t = torch.zeros(8)
    for s in AC.betas_table() + AC.split_table(17):
        if s.mode == AC.DENSE:
            d = W.adam_desc(W.ADAM_DENSE, t, t, t, t, s.lr, s.betas[0], s.betas[1], s.eps, step=float(s.step))
            got = (d.one_minus_beta1, d.beta2, d.one_minus_beta2, -d.step_size, d.bias_correction2_sqrt, d.eps)
            assert got == tuple(float(x) for x in AC.dense_constants(s)), s
        else:
            vis = torch.ones(4, dtype=torch.bool)
            d = W.adam_desc(W.ADAM_SELECTIVE, t, t, t, t, s.lr, s.betas[0], s.betas[1], s.eps, visibility=vis, rows=4, row_width=2, n=8)
            assert (d.lr, d.beta1, d.beta2, d.eps) == tuple(float(x) for x in AC.selective_constants(s)), s
    assert (AC.DENSE, AC.SELECTIVE, AC.TABLE_MAX) == (W.ADAM_DENSE, W.ADAM_SELECTIVE, int(W.B.query("gs_adam_multi_max")))


def test_restatement_against_float64_on_every_named_table():
    """Prints the largest relative error of the float32 restatement against the float64 oracle, per array and table (the figures of
    adam_cases' docstring).  exp_avg_sq is a sum of non-negative terms, so its error is the roundings (3 of 2^-24) plus the
    constants': 1 - float32(0.999) against 0.001 is 3e-5 off in the selective mode, nothing else comes near -- hence < 1e-4.
    exp_avg and p can cancel and have no a-priori bound; they have to be finite."""
    for name, specs in AC.named_tables():
        worst = [0.0, 0.0, 0.0]
        for case in AC.build_table(specs, AC.table_rng(name)):
            for k, (a, b) in enumerate(zip(AC.restate_f32(case), AC.oracle_f64(case))):
                worst[k] = max(worst[k], AC.rel_err(a, b))
        print(f"    {name:<26} {worst[0]:.2e}   {worst[1]:.2e}   {worst[2]:.2e}")
        assert all(np.isfinite(w) for w in worst) and worst[2] < 1e-4, (name, worst)


def test_restatement_branches_and_untouched_rows():
    """The second lerp branch is taken from |1 - beta1| >= 0.5 on (beta1 = 0 gives exp_avg = g exactly, which the first branch
    does not), and selective_f32 returns the old bits for the rows that are not visible."""
    rng = np.random.default_rng(3)
    case = AC.build_table([AC.Spec(AC.DENSE, 1000, betas=(0.0, 0.5))], rng)[0]
    _, m1, _ = AC.restate_f32(case)
    assert np.array_equal(AC.bits(m1), AC.bits(case.data("g") + np.float32(0)))  # (-0 + 0 = +0, as g - (g - m) * 0 gives)
    m, g = case.data("m"), case.data("g")
    assert not np.array_equal(m + np.float32(1) * (g - m), m1)
    case = AC.build_table([AC.Spec(AC.SELECTIVE, 35, row_width=5, vis="alt")], rng)[0]
    keep = np.repeat(case.vis != 0, 5)
    assert keep.tolist() == ([True] * 5 + [False] * 5) * 3 + [True] * 5
    for new, name in zip(AC.restate_f32(case), ("p", "m", "v")):
        old = case.data(name)
        assert np.array_equal(AC.bits(new)[~keep], AC.bits(old)[~keep]) and not (AC.bits(new)[keep] == AC.bits(old)[keep]).any()


def test_build_table_offsets_sentinels_and_disjoint_arrays():
    specs = AC.split_table(17, with_empty=True) + AC.edge_table_mismatched() + AC.selective_table(3)[:8]
    cases = AC.build_table(specs, np.random.default_rng(5))
    assert len(cases) == len(specs)
    views = []
    for case in cases:
        s = case.spec
        for name, off in zip(AC.ARRAYS, s.offsets):
            buf = case.padded[name]
            assert buf.dtype == np.float32 and buf.size == s.n + 2 * AC.PAD
            assert case.data(name).ctypes.data % 16 == off if s.n else True, (s, name)
            assert buf.ctypes.data % 16 == off
            assert (AC.bits(buf[:AC.PAD]) == AC.SENTINEL_BITS).all() and (AC.bits(buf[AC.PAD + s.n:]) == AC.SENTINEL_BITS).all()
            assert np.isfinite(buf).all() and not (AC.bits(case.data(name)) == AC.SENTINEL_BITS).any()
            views.append(buf)
        p, g, m, v = (case.data(k) for k in AC.ARRAYS)
        assert ((np.abs(p) >= 0.1) & (np.abs(p) <= 2)).all() and ((np.abs(m) >= np.float32(1e-3)) & (np.abs(m) <= 1)).all()
        nz = np.abs(g[g != 0])
        assert int((g == 0).sum()) == s.n // 20 and ((nz >= np.float32(1e-3)) & (nz <= 1)).all()
        if s.zero_v:
            assert (g == 0).any() and ((v == 0) == (g == 0)).all()
        else:
            assert ((v >= np.float32(1e-6)) & (v <= 1)).all()
        if s.mode == AC.SELECTIVE:
            assert case.vis.dtype == np.uint8 and case.vis.size == s.rows and s.rows * s.row_width == s.n
        else:
            assert case.vis is None
    spans = sorted((b.ctypes.data, b.ctypes.data + b.nbytes) for b in views)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "two arrays overlap"
    assert sum(s.zero_v for s in specs[:17]) == 1 and [i for i, s in enumerate(specs[:17]) if s.n == 0] == [0, 15, 16]


def test_named_tables_are_what_the_gpu_test_says_they_are():
    assert len(AC.edge_table(0)) == len(AC.EDGE_SIZES) == 15 and all(len(set(s.offsets)) == 1 for h in range(4) for s in AC.edge_table(h))
    assert {s.offsets[0] for h in range(4) for s in AC.edge_table(h)} == {0, 4, 8, 12}
    assert all(len(set(s.offsets)) > 1 for s in AC.edge_table_mismatched())
    # a tensor that is all head (n below the head size) and the c == 0 -> 1 rule; n - head an exact multiple of a quad / a chunk
    assert [AC.chunks_of(s) for s in AC.edge_table(3)[:3]] == [1, 1, 1]
    sizes = {s.n - h for h in range(4) for s in AC.edge_table(h)}
    assert {3 * AC.CHUNK, 3 * AC.CHUNK - 1, 3 * AC.CHUNK + 1, 1024, 4}.issubset(sizes)
    for o in (0, 3, "mismatched"):
        t = AC.selective_table(o)
        assert len(t) == 36 and all(3000 <= s.n <= 6000 and s.rows * s.row_width == s.n for s in t)
        assert {s.row_width for s in t} == set(AC.SELECTIVE_WIDTHS) and sum(s.zero_v for s in t) == 1
    assert len(AC.betas_table()) == 24 and {s.betas for s in AC.betas_table()} == set(AC.BETAS)
    for c in AC.SPLIT_COUNTS:
        for e in (False, True):
            t = AC.split_table(c, e)
            assert len(t) == c and [s.mode for s in t] == [i % 2 for i in range(c)]
            assert len({(s.lr, s.betas, s.eps, s.step) for s in t if not s.zero_v}) == sum(not s.zero_v for s in t)
            assert [i for i, s in enumerate(t) if s.n == 0] == (sorted({0, 15, 16, c - 1} & set(range(c))) if e else [])
    many = AC.many_chunks_table()
    assert len(many) == 40 and all(AC.chunks_of(s) == 69 for s in many)
