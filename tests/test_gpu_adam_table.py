"""gs_adam_multi (csrc/optim.hip) on the paths that depend on the data: tables of more than GS_ADAM_MULTI_MAX descriptors, n == 0
descriptors, a bad descriptor behind the first table, heads of 0-3 elements and tensors that are all head, mismatched offsets
(every element scalar) in both modes, chunk and quad edges, row widths across the three regimes of the reciprocal division with
quads that straddle rows, the second lerp branch (beta1 <= 0.5), and a grid that strides over many small tensors.

Every call is held to tests/adam_cases.py: the float32 restatement (rtol 1e-6, atol 1e-7 / 1e-6 / 1e-9 for p / exp_avg /
exp_avg_sq), the float64 oracle (per descriptor and array: at most twice the restatement's own distance plus one float32 ulp),
sentinels around all four arrays, the gradient and the invisible rows bit-identical."""
import numpy as np
import pytest
import torch

import adam_cases as AC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
RTOL = 1e-6
ATOL = {"p": 1e-7, "m": 1e-6, "v": 1e-9}
OUT = ("p", "m", "v")


def _W():
    from gscodec_studio_amd import _wrapper as W

    return W


def _upload(host, offset):
    """A device copy of a padded host buffer, its data ``offset`` bytes past a 16-byte boundary (PAD floats are 32 bytes)."""
    store = torch.empty(host.size + 4, dtype=torch.float32, device=DEV)
    k = AC.slice_start(store.data_ptr(), offset)
    t = store[k:k + host.size]
    t.copy_(torch.from_numpy(np.ascontiguousarray(host)))
    assert t.data_ptr() % 16 == offset
    return t


class _Device:
    """The cases of a table on the device, and one descriptor each."""

    def __init__(self, cases):
        W = _W()
        self.cases = cases
        self.padded, self.vis, self.descs = [], [], []
        empty, no_vis = torch.empty(0, dtype=torch.float32, device=DEV), torch.empty(0, dtype=torch.bool, device=DEV)
        for case in cases:
            s = case.spec
            if s.n == 0:  # null pointers: the call has to pass over it
                bufs, data, vis = None, {k: empty for k in AC.ARRAYS}, no_vis
            else:
                bufs = {k: _upload(case.padded[k], off) for k, off in zip(AC.ARRAYS, s.offsets)}
                data = {k: b[AC.PAD:AC.PAD + s.n] for k, b in bufs.items()}
                for k, off in zip(AC.ARRAYS, s.offsets):
                    assert data[k].data_ptr() % 16 == off and data[k].numel() == s.n
                vis = torch.from_numpy(case.vis).to(DEV).view(torch.bool) if s.mode == AC.SELECTIVE else None
            if s.mode == AC.SELECTIVE:
                d = W.adam_desc(W.ADAM_SELECTIVE, data["p"], data["g"], data["m"], data["v"], s.lr, s.betas[0], s.betas[1], s.eps,
                                visibility=vis, rows=s.rows, row_width=s.row_width, n=s.n)
            else:
                d = W.adam_desc(W.ADAM_DENSE, data["p"], data["g"], data["m"], data["v"], s.lr, s.betas[0], s.betas[1], s.eps,
                                step=float(s.step))
            if s.n == 0:
                assert d.n == 0 and d.param is None and d.grad is None and d.exp_avg is None and d.exp_avg_sq is None
            self.padded.append(bufs)
            self.vis.append(vis)
            self.descs.append(d)

    def like(self):
        return next(b["p"] for b in self.padded if b is not None)

    def step(self, one_call=True):
        W = _W()
        if one_call:
            W.adam_multi(self.descs, self.like())
        else:
            for d in self.descs:
                W.adam_multi([d], self.like())
        torch.cuda.synchronize()

    def download(self):
        return [None if b is None else {k: t.cpu().numpy() for k, t in b.items()} for b in self.padded]


def _constants(d, mode):
    """The float constants exactly as the descriptor carries them."""
    if mode == AC.SELECTIVE:
        return dict(selective_c=(d.lr, d.beta1, d.beta2, d.eps))
    return dict(dense_c=(d.one_minus_beta1, d.beta2, d.one_minus_beta2, -d.step_size, d.bias_correction2_sqrt, d.eps))


def _check_untouched(dev, got=None):
    """Every array of every tensor bit-identical to what was uploaded, sentinels included."""
    got = dev.download() if got is None else got
    for i, (case, g) in enumerate(zip(dev.cases, got)):
        for k in AC.ARRAYS if g is not None else ():
            assert np.array_equal(AC.bits(g[k]), AC.bits(case.padded[k])), f"descriptor {i}: {k} changed"


def _check(dev, name):
    """The common checks after one step of a freshly uploaded table.  Returns what was downloaded."""
    got = dev.download()
    worst = {k: [0.0, 0.0] for k in OUT}  # array -> [kernel, restatement] against float64, largest over the table
    off_by_bits = 0
    for i, (case, g, d) in enumerate(zip(dev.cases, got, dev.descs)):
        s = case.spec
        if g is None:
            continue
        what = f"{name}, descriptor {i} ({'selective' if s.mode else 'dense'}, n = {s.n}, offsets {s.offsets}, width {s.row_width})"
        for k in AC.ARRAYS:
            pad = np.concatenate([AC.bits(g[k][:AC.PAD]), AC.bits(g[k][AC.PAD + s.n:])])
            assert (pad == AC.SENTINEL_BITS).all(), f"{what}: a store outside {k}"
        assert np.array_equal(AC.bits(g["g"]), AC.bits(case.padded["g"])), f"{what}: the gradient changed"
        want = dict(zip(OUT, AC.restate_f32(case, **_constants(d, s.mode))))
        ref64 = dict(zip(OUT, AC.oracle_f64(case)))
        for k in OUT:
            x = g[k][AC.PAD:AC.PAD + s.n]
            if s.mode == AC.SELECTIVE:
                hidden = ~np.repeat(case.vis != 0, s.row_width)
                assert np.array_equal(AC.bits(x)[hidden], AC.bits(case.data(k))[hidden]), f"{what}: an invisible row of {k} changed"
            np.testing.assert_allclose(x, want[k], rtol=RTOL, atol=ATOL[k], err_msg=f"{what}: {k} against the float32 restatement")
            off_by_bits += int((AC.bits(x) != AC.bits(want[k])).sum())
            e_kernel, e_restated = AC.rel_err(x, ref64[k]), AC.rel_err(want[k], ref64[k])
            assert e_kernel <= 2 * e_restated + AC.ULP, (f"{what}: {k} is {e_kernel:.3e} from the float64 oracle, the float32 "
                                                           f"restatement {e_restated:.3e}")
            worst[k] = [max(worst[k][0], e_kernel), max(worst[k][1], e_restated)]
    print(f"[{name}] largest relative error against float64, kernel / restatement: "
          + ", ".join(f"{k} {worst[k][0]:.2e} / {worst[k][1]:.2e}" for k in OUT)
          + f"; {off_by_bits} elements differ in bits from the restatement")
    return got


def _run(name, specs=None):
    specs = dict(AC.named_tables())[name] if specs is None else specs
    dev = _Device(AC.build_table(specs, AC.table_rng(name)))
    dev.step()
    return dev, _check(dev, name)


@pytest.mark.parametrize("head", [0, 1, 2, 3, "mismatched"])
def test_edge_sizes_and_heads(head):
    """EDGE_SIZES in dense mode, one table per head (all four arrays 0 / 12 / 8 / 4 bytes past a 16-byte boundary; sizes 1-3 are
    all head, or below it), and the four MISMATCHED_SIZES at four mixtures of offsets (vec == 0: every element scalar)."""
    _run("edge mismatched" if head == "mismatched" else f"edge head {head}")


@pytest.mark.parametrize("offsets", [0, 3, "mismatched"])
def test_selective_row_widths(offsets):
    """SELECTIVE_WIDTHS (l = 0, powers of two, others; quads over two, three and four rows) x visibility 0 / 0.25 / 1 /
    alternating, with equal offsets at heads 0 and 3 and with mismatched offsets."""
    _run("selective mismatched" if offsets == "mismatched" else f"selective head {offsets}")


def test_low_beta1_takes_the_second_lerp_branch():
    """BETAS x step {1, 2, 1000} x eps {1e-15, 1e-8}: through the C ABI against the restatement and the oracle, then the same
    cases through optimizers.Adam (one group per case, one step from a seeded state) against torch.optim.Adam(foreach=False)."""
    from gscodec_studio_amd.optimizers import Adam

    dev, _ = _run("betas")
    assert sum(abs(d.one_minus_beta1) >= 0.5 for d in dev.descs) == 18  # three of the four BETAS take the second branch

    def optimizer(cls, **kw):
        params, groups = [], []
        for case in dev.cases:
            p = torch.nn.Parameter(torch.tensor(case.data("p"), device=DEV))
            p.grad = torch.tensor(case.data("g"), device=DEV)
            params.append(p)
            groups.append({"params": [p], "lr": case.spec.lr, "betas": case.spec.betas, "eps": case.spec.eps})
        opt = cls(groups, **kw)
        for p, case in zip(params, dev.cases):
            opt.state[p] = {"step": torch.tensor(float(case.spec.step - 1)), "exp_avg": torch.tensor(case.data("m"), device=DEV),
                            "exp_avg_sq": torch.tensor(case.data("v"), device=DEV)}
        opt.step()
        return params, opt

    (pa, oa), (pt, ot) = optimizer(Adam), optimizer(torch.optim.Adam, foreach=False)
    torch.cuda.synchronize()
    for case, a, t in zip(dev.cases, pa, pt):
        sa, st = oa.state[a], ot.state[t]
        assert float(sa["step"]) == float(st["step"]) == case.spec.step
        torch.testing.assert_close(a.detach(), t.detach(), rtol=RTOL, atol=ATOL["p"], msg=lambda m: f"{case.spec}: p\n{m}")
        torch.testing.assert_close(sa["exp_avg"], st["exp_avg"], rtol=RTOL, atol=ATOL["m"], msg=lambda m: f"{case.spec}: exp_avg\n{m}")
        torch.testing.assert_close(sa["exp_avg_sq"], st["exp_avg_sq"], rtol=RTOL, atol=ATOL["v"],
                                   msg=lambda m: f"{case.spec}: exp_avg_sq\n{m}")


@pytest.mark.parametrize("with_empty", [False, True])
@pytest.mark.parametrize("count", AC.SPLIT_COUNTS)
def test_table_split(count, with_empty):
    """More descriptors than one launch takes: every tensor is stepped exactly once with its own constants (the common checks: a
    second step, a skipped one or a neighbour's constants all miss the restatement), and the table submitted as one call equals
    one call per descriptor bit for bit.  with_empty: n == 0 descriptors with null pointers at positions 0, 15, 16 and last."""
    name = f"split {count}{' with empty' if with_empty else ''}"
    dev, got = _run(name)
    single = _Device(dev.cases)
    single.step(one_call=False)
    for i, (a, b) in enumerate(zip(got, single.download())):
        for k in AC.ARRAYS if a is not None else ():
            assert np.array_equal(AC.bits(a[k]), AC.bits(b[k])), f"{name}, descriptor {i}: {k} differs between one call and a call of its own"


def test_a_table_of_empty_descriptors_is_a_no_op():
    """n == 0 descriptors as the whole table, and as a whole table (16) in front of one tensor."""
    W = _W()
    dev = _Device(AC.build_table([AC.Spec(AC.DENSE, 0), AC.Spec(AC.SELECTIVE, 0, row_width=3), AC.Spec(AC.DENSE, 0)], AC.table_rng("empty")))
    W.adam_multi(dev.descs, torch.empty(1, device=DEV))
    torch.cuda.synchronize()
    _run("empty table first", [AC.Spec(AC.DENSE, 0)] * AC.TABLE_MAX + [AC.Spec(AC.DENSE, 1027, AC.head_offsets(1), lr=2e-3, step=3)])


@pytest.mark.parametrize("one_launch", [False, True])
def test_many_small_tensors_under_the_grid_cap(one_launch):
    """MANY_CHUNKS: 40 tensors of 69 chunks, more chunks in total than the grid has blocks -- but the split hands the kernel 16
    tensors (1 104 chunks) at a time, so on a device whose cap exceeds 1 104 no block skips a tensor: this variant is kept because
    the issue behind this module names it, and its skip condition is the issue's (chunks of the whole table).
    MANY_CHUNKS_ONE_LAUNCH is the one that does the job: 16 tensors of 137 chunks, more than the grid has blocks within one
    launch, so a block's stride carries it over whole tensors (``while (c >= a.chunk_end[t]) ++t`` more than once)."""
    props = torch.cuda.get_device_properties(DEV)
    cap = props.multi_processor_count * (props.max_threads_per_multi_processor // AC.BLOCK)  # optim.hip's device_grid_cap
    specs = AC.many_chunks_table(one_launch)
    chunks = sum(AC.chunks_of(s) for s in specs)
    assert chunks == len(specs) * (137 if one_launch else 69)
    if chunks <= cap:
        pytest.skip(f"{chunks} chunks do not exceed this device's grid cap of {cap} blocks")
    _run("many chunks in one launch" if one_launch else "many chunks", specs)


@pytest.mark.parametrize("way", ["unknown mode", "rows * row_width != n", "null grad", "pointer % 4 != 0"])
def test_bad_descriptor_behind_the_first_table_leaves_everything_untouched(way):
    """20 valid descriptors, number 18 made invalid: the call raises naming it, and nothing was launched for the 16 before it."""
    W = _W()
    specs = AC.split_table(21)[1:]  # (number 18 is a selective one)
    assert len(specs) == 20 and specs[18].mode == AC.SELECTIVE and specs[18].n > 0
    dev = _Device(AC.build_table(specs, AC.table_rng("bad descriptor")))
    descs = [W._AdamDesc.from_buffer_copy(d) for d in dev.descs]
    bad = descs[18]
    if way == "unknown mode":
        bad.mode = 7
    elif way == "rows * row_width != n":
        bad.rows += 1
    elif way == "null grad":
        bad.grad = None
    else:
        bad.param = bad.param + 2  # never dereferenced: the host refuses it
        assert bad.param % 4 == 2
    with pytest.raises(RuntimeError, match="descriptor 18"):
        W.adam_multi(descs, dev.like())
    torch.cuda.synchronize()
    _check_untouched(dev)
    dev.step()  # the same table, valid: it does step (the check above would pass for a call that never launches)
    _check(dev, "bad descriptor, then valid")


def test_step_all_with_more_parameters_than_one_table():
    """40 parameters of EDGE_SIZES sizes over optimizers.Adam, torch.optim.Adam (three groups each, own lr / betas) and three
    SelectiveAdam (visibility of 50 rows: M = numel // 50, smaller parameters are passed over), stepped twice by step_all, against
    each optimizer stepped on its own through this package's step (optimizers.Adam in torch.optim.Adam's place, as in
    test_step_all_batches_bit_identically): bit-identical parameters and states, dense step counters 2, selective ones 0."""
    from gscodec_studio_amd.optimizers import Adam, SelectiveAdam, step_all

    rows = 50
    vis = torch.from_numpy(np.arange(rows) % 3 != 1).to(DEV)

    def build(dense_classes):
        rng = np.random.default_rng(17)
        params = []
        for i in range(40):
            n = AC.EDGE_SIZES[i % len(AC.EDGE_SIZES)]
            base = torch.tensor(rng.uniform(0.1, 2.0, n + 3).astype(np.float32), device=DEV)
            params.append(torch.nn.Parameter(base[i % 4:i % 4 + n]))  # (the moments are aligned: mismatched offsets for i % 4 != 0)
        owners = [[p for i, p in enumerate(params) if i % 5 == k] for k in range(5)]
        opts = []
        for k, cls in enumerate(dense_classes):
            groups = [{"params": owners[k][j::3], "lr": 1e-3 * (1 + j + 3 * k), "betas": AC.BETAS[(j + k) % 4], "eps": AC.BETAS_EPS[j % 2]}
                      for j in range(3)]
            opts.append(cls(groups))
        for k in (2, 3, 4):
            opts.append(SelectiveAdam([{"params": [p], "lr": 1e-3 * (1 + j + k)} for j, p in enumerate(owners[k])], eps=1e-15,
                                      betas=AC.BETAS[k % 4]))
        return params, opts

    def grads(params, step):
        rng = np.random.default_rng(100 + step)
        for p in params:
            p.grad = torch.tensor((rng.standard_normal(p.numel()) * 0.3).astype(np.float32), device=DEV)

    pa, oa = build((Adam, torch.optim.Adam))
    pb, ob = build((Adam, Adam))
    first = [p.detach().clone() for p in pa]
    for step in range(2):
        grads(pa, step)
        grads(pb, step)
        step_all(oa, visibility=vis)
        assert all(p.grad is None for p in pa)
        for o in ob[:2]:
            o.step()
        for o in ob[2:]:
            o.step(vis)
    torch.cuda.synchronize()
    stepped = 0
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32)), f"parameter {i}"
        sa, sb = oa[i % 5].state[a], ob[i % 5].state[b]
        selective = i % 5 >= 2
        if selective and a.numel() < rows:  # M == 0: passed over, by step_all and by step() alike
            continue
        stepped += 1
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(sa[k].view(torch.int32), sb[k].view(torch.int32)), f"parameter {i}: {k}"
        assert float(sa["step"]) == float(sb["step"]) == (0.0 if selective else 2.0), f"parameter {i}"
        assert not torch.equal(a.detach(), first[i]), f"parameter {i} was not stepped"
    assert stepped > AC.TABLE_MAX  # (more descriptors than one launch takes)

