"""gs_sparse_adam_multi (csrc/optim.hip) through the C entry on the named calls of tests/sparse_adam_cases.py, then
optimizers.SparseAdam, step_all's batching, densification and the packed sparse-gradient render, each against
torch.optim.SparseAdam on the same device.

C entry: sentinels around p, exp_avg, exp_avg_sq and values, every row without an index and the values bit-identical afterwards,
the touched elements within twice the float32 restatement's own distance from the float64 oracle plus one float32 ulp (per
descriptor and array), and two runs of the same call bit-identical.  No call passes an id outside [0, rows)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import adam_cases as AC
import sparse_adam_cases as SC
from util import T, garden

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LRS = {"means": 1.6e-4, "scales": 5e-3, "quats": 1e-3, "opacities": 5e-2, "sh0": 2.5e-3, "shN": 2.5e-3 / 20}
SHAPES = {"means": (3,), "scales": (3,), "quats": (4,), "opacities": (), "sh0": (1, 3), "shN": (15, 3)}  # config 2's splat set


def _S():
    from gscodec_studio_amd.optimizers import sparse as S

    return S


def _upload(host, offset):
    store = torch.empty(host.size + 4, dtype=torch.float32, device=DEV)
    k = AC.slice_start(store.data_ptr(), offset)
    t = store[k:k + host.size]
    t.copy_(torch.from_numpy(np.ascontiguousarray(host)))
    assert t.data_ptr() % 16 == offset
    return t


class _Device:
    """One case on the device and one descriptor per tensor."""

    def __init__(self, case):
        S = _S()
        call = self.call = case.call
        self.case = case
        self.sorted_ids = torch.from_numpy(case.sorted_ids).to(DEV)
        self.perm = None if case.perm is None else torch.from_numpy(case.perm).to(DEV)
        self.padded, self.descs = [], []
        for i, d in enumerate(call.descs):
            bufs = {k: _upload(case.padded[i][k], d.values_offset if k == "g" else 0) for k in ("p", "m", "v", "g")}
            n, ng = call.rows * d.row_width, call.nnz * d.row_width
            data = {k: b[AC.PAD:AC.PAD + (ng if k == "g" else n)] for k, b in bufs.items()}
            assert ng == 0 or data["g"].data_ptr() % 16 == d.values_offset
            self.padded.append(bufs)
            self.descs.append(S.sparse_adam_desc(data["p"], data["m"], data["v"], data["g"], d.row_width, d.lr, d.betas[0], d.betas[1],
                                                 d.eps, d.step))

    def step(self, one_call=True):
        S = _S()
        for descs in ([self.descs] if one_call else [[d] for d in self.descs]):
            if self.call.nnz == 0:  # (the wrapper returns before the call: straight to the C entry, which launches nothing)
                table = (S.sparse_adam_desc_class() * len(descs))(*descs)
                S.B.call("gs_sparse_adam_multi", len(descs), ctypes.addressof(table), 0, None, None, self.call.rows, S.W._stream(self.padded[0]["p"]))
                continue
            S.sparse_adam_multi(descs, self.call.nnz, self.sorted_ids, self.perm, self.call.rows, self.padded[0]["p"])
        torch.cuda.synchronize()
        return [{k: t.cpu().numpy() for k, t in b.items()} for b in self.padded]


def _check(case, dev, got):
    call = case.call
    worst = {k: [0.0, 0.0] for k in SC.OUT}
    off_by_bits = 0
    for i, (d, g, desc) in enumerate(zip(call.descs, got, dev.descs)):
        what = f"{call.name}, descriptor {i} (width {d.row_width}, values offset {d.values_offset})"
        n = call.rows * d.row_width
        for k in ("p", "m", "v", "g"):
            size = call.nnz * d.row_width if k == "g" else n
            pad = np.concatenate([AC.bits(g[k][:AC.PAD]), AC.bits(g[k][AC.PAD + size:])])
            assert (pad == AC.SENTINEL_BITS).all(), f"{what}: a store outside {k}"
        assert np.array_equal(AC.bits(g["g"]), AC.bits(case.padded[i]["g"])), f"{what}: the values changed"
        c = (desc.one_minus_beta1, desc.one_minus_beta2, desc.neg_step_size, desc.eps)  # exactly as the descriptor carries them
        want = dict(zip(SC.OUT, case.restate_f32(i, c)))
        ref64 = dict(zip(SC.OUT, case.oracle_f64(i)))
        touched = case.touched(i)
        for k in SC.OUT:
            x = g[k][AC.PAD:AC.PAD + n]
            assert np.array_equal(AC.bits(x)[~touched], AC.bits(case.data(i, k).ravel())[~touched]), f"{what}: a row of {k} without an index changed"
            xt, wt, rt = x[touched], want[k].ravel()[touched], ref64[k].ravel()[touched]
            if call.nnz:
                assert not np.array_equal(xt, case.data(i, k).ravel()[touched]), f"{what}: {k} was not stepped"
            off_by_bits += int((AC.bits(xt) != AC.bits(wt)).sum())
            e_kernel, e_restated = AC.rel_err(xt, rt), AC.rel_err(wt, rt)
            assert e_kernel <= 2 * e_restated + AC.ULP, (f"{what}: {k} is {e_kernel:.3e} from the float64 oracle, the float32 "
                                                           f"restatement {e_restated:.3e}")
            worst[k] = [max(worst[k][0], e_kernel), max(worst[k][1], e_restated)]
    print(f"[{call.name}] largest relative error against float64, kernel / restatement: "
          + ", ".join(f"{k} {worst[k][0]:.2e} / {worst[k][1]:.2e}" for k in SC.OUT)
          + f"; {off_by_bits} elements differ in bits from the restatement")


def _run(call):
    case = SC.build_call(call, SC.call_rng(call.name))
    dev = _Device(case)
    got = dev.step()
    _check(case, dev, got)
    again = _Device(case).step()
    for i, (a, b) in enumerate(zip(got, again)):
        for k in a:
            assert np.array_equal(AC.bits(a[k]), AC.bits(b[k])), f"{call.name}, descriptor {i}: {k} differs between two runs"
    return case, got


@pytest.mark.parametrize("nnz", SC.NNZ)
@pytest.mark.parametrize("rows", SC.ROWS)
def test_table_through_the_c_entry(rows, nnz):
    """ROW_WIDTHS in one call per index pattern that fits (rows, nnz): sorted unique with perm = NULL, shuffled unique, every id
    twice, run lengths 1..4, random ids (the only pattern with more indices than rows: long runs); ids 0 and rows - 1 present, the
    values' base pointers at byte offsets 0 / 4 / 8 / 12 mod 16.  nnz == 0 launches nothing and leaves everything as it was."""
    calls = SC.grid_calls(rows, nnz)
    assert calls
    for call in calls:
        _run(call)


@pytest.mark.parametrize("name", [c.name for c in SC.special_calls()])
def test_special_calls_through_the_c_entry(name):
    """A run of 300 (at row_width 1 it crosses a 256-lane workgroup), runs that start at sorted position 0 and end at nnz - 1, and
    17 descriptors in one call (two launches), which also equals one call per descriptor bit for bit."""
    call = next(c for c in SC.special_calls() if c.name == name)
    case, got = _run(call)
    if len(call.descs) > SC.TABLE_MAX:
        single = _Device(case).step(one_call=False)
        for i, (a, b) in enumerate(zip(got, single)):
            for k in a:
                assert np.array_equal(AC.bits(a[k]), AC.bits(b[k])), f"{name}, descriptor {i}: {k} differs from a call of its own"


# ------------------------------------------------------------------------------------------------------------------------------
# optimizer level
# ------------------------------------------------------------------------------------------------------------------------------
def _ulp(a, b):
    """Largest distance in float32 ulps over the elements with |b| >= 2^-10 (next to zero an ulp count says nothing)."""
    keep = b.abs() >= 2.0 ** -10
    a, b = a[keep], b[keep]
    ai, bi = a.contiguous().view(torch.int32).long(), b.contiguous().view(torch.int32).long()
    ai = torch.where(ai < 0, -(ai & 0x7FFFFFFF), ai)
    bi = torch.where(bi < 0, -(bi & 0x7FFFFFFF), bi)
    return int((ai - bi).abs().max()) if ai.numel() else 0


def _assert_state_close(ours, ref, p_ours, p_ref, rtol=1e-6, p_atol=1e-7):
    """test_gpu_optimizers.py::_assert_state_close with SparseAdam's step (a Python int)."""
    torch.testing.assert_close(p_ours.detach(), p_ref.detach(), rtol=rtol, atol=p_atol)
    so, sr = ours.state[p_ours], ref.state[p_ref]
    torch.testing.assert_close(so["exp_avg"], sr["exp_avg"], rtol=rtol, atol=1e-6)
    torch.testing.assert_close(so["exp_avg_sq"], sr["exp_avg_sq"], rtol=rtol, atol=1e-9)
    assert isinstance(so["step"], int) and so["step"] == sr["step"]
    return max(_ulp(p_ours.detach(), p_ref.detach()), _ulp(so["exp_avg"], sr["exp_avg"]), _ulp(so["exp_avg_sq"], sr["exp_avg_sq"]))


def _params(n, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return {k: torch.nn.Parameter(torch.rand((n, *s), device=DEV, generator=g) * 2 - 1) for k, s in SHAPES.items()}


def _clone(ps):
    return {k: torch.nn.Parameter(p.detach().clone()) for k, p in ps.items()}


def _opts(ps, cls):
    return {k: cls([{"params": [p], "lr": LRS[k], "name": k}], eps=1e-15, betas=(0.9, 0.999)) for k, p in ps.items()}


def _ids(n, nnz, rng, coalesced=False):
    """int64 [nnz] on the device, at most two duplicates per id (torch's own sum of two has one order only)."""
    if coalesced:
        return torch.from_numpy(np.sort(rng.permutation(n)[:nnz])).to(DEV)
    uniq = rng.permutation(n)[:nnz - nnz // 3]
    return torch.from_numpy(rng.permutation(np.concatenate([uniq, uniq[:nnz // 3]]))).to(DEV)


def _set_grads(targets, ids, seed, coalesced=False, share=True, keys=None):
    """The same sparse gradients (cloned values) on every dict of ``targets`` (for ``keys``, default all); share: one index
    tensor for all of a dict."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    for k, s in SHAPES.items():
        values = torch.randn((ids.numel(), *s), device=DEV, generator=g) * 0.3
        for ps in targets if keys is None or k in keys else ():
            idx = ids if share else ids.clone()
            ps[k].grad = torch.sparse_coo_tensor(idx[None], values.clone(), ps[k].shape, is_coalesced=coalesced)


def _compare(oa, ob, pa, pb, what):
    worst = max(_assert_state_close(oa[k], ob[k], pa[k], pb[k]) for k in pa)
    print(f"[{what}] worst distance from torch.optim.SparseAdam: {worst} ulp")
    return worst


def test_sparse_adam_matches_torch():
    """optimizers.SparseAdam against torch.optim.SparseAdam, 5 steps with fresh indices (one of them coalesced), then a step with
    an empty gradient (the step counter advances, nothing else moves), then state_dict both ways and a further step."""
    from gscodec_studio_amd.optimizers import SparseAdam

    n, rng = 1500, np.random.default_rng(5)
    ps0 = _params(n)
    pa, pb = _clone(ps0), _clone(ps0)
    oa, ob = _opts(pa, SparseAdam), _opts(pb, torch.optim.SparseAdam)
    for step in range(5):
        coalesced = step == 3
        _set_grads((pa, pb), _ids(n, 700, rng, coalesced), step, coalesced)
        for o in list(oa.values()) + list(ob.values()):
            o.step()
    torch.cuda.synchronize()
    _compare(oa, ob, pa, pb, "5 steps")
    for k in pa:
        assert not torch.equal(pa[k].detach(), ps0[k].detach())

    before = {k: (pa[k].detach().clone(), oa[k].state[pa[k]]["exp_avg"].clone(), oa[k].state[pa[k]]["exp_avg_sq"].clone()) for k in pa}
    _set_grads((pa, pb), torch.zeros(0, dtype=torch.int64, device=DEV), 9)
    for o in list(oa.values()) + list(ob.values()):
        o.step()
    for k in pa:
        st = oa[k].state[pa[k]]
        assert st["step"] == ob[k].state[pb[k]]["step"] == 6
        for a, b in zip(before[k], (pa[k].detach(), st["exp_avg"], st["exp_avg_sq"])):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k

    # torch's optimizer continues from ours and ours from torch's
    pc, pd = _clone(pa), _clone(pb)
    oc, od = _opts(pc, torch.optim.SparseAdam), _opts(pd, SparseAdam)
    for k in pa:
        oc[k].load_state_dict(copy.deepcopy(oa[k].state_dict()))  # (load_state_dict keeps the tensors it is given)
        od[k].load_state_dict(copy.deepcopy(ob[k].state_dict()))
        assert oc[k].state[pc[k]]["step"] == od[k].state[pd[k]]["step"] == 6
    _set_grads((pa, pb, pc, pd), _ids(n, 700, rng), 11)
    for o in (*oa.values(), *ob.values(), *oc.values(), *od.values()):
        o.step()
    torch.cuda.synchronize()
    _compare(oa, ob, pa, pb, "after an empty step")
    _compare(oa, oc, pa, pc, "torch's from our state")
    _compare(od, ob, pd, pb, "ours from torch's state")
    assert od["means"].state[pd["means"]]["step"] == 7


def test_single_row_parameter_needs_no_sort():
    """rows == 1: no key bits to sort on, the indices are all 0 and in order as they stand."""
    from gscodec_studio_amd.optimizers import SparseAdam

    pa = torch.nn.Parameter(torch.tensor([[0.5, -1.0, 2.0, 0.25]], device=DEV))
    pb = torch.nn.Parameter(pa.detach().clone())
    oa, ob = SparseAdam([pa], lr=1e-2, eps=1e-15), torch.optim.SparseAdam([pb], lr=1e-2, eps=1e-15)
    for p in (pa, pb):
        p.grad = torch.sparse_coo_tensor(torch.zeros(1, 2, dtype=torch.int64, device=DEV),
                                         torch.tensor([[0.1, 0.2, -0.3, 0.0], [0.05, -0.2, 0.4, 0.0]], device=DEV), p.shape)
    oa.step()
    ob.step()
    _assert_state_close(oa, ob, pa, pb)
    assert not torch.equal(pa.detach()[0, :3], torch.tensor([0.5, -1.0, 2.0], device=DEV))


def test_step_all_batches_bit_identically():
    """Six SparseAdam over one shared index list plus a dense Adam in one step_all call: one sort, one sparse launch, one dense
    launch, and every bit as from each optimizer's own step().  Second step: the index lists do not share storage (a group
    each); third: two lists of different length in one call."""
    from gscodec_studio_amd import _backend
    from gscodec_studio_amd.optimizers import Adam, SparseAdam, step_all
    from gscodec_studio_amd.optimizers import sparse as S

    n, rng = 1500, np.random.default_rng(6)
    ps0 = _params(n, seed=1)
    extra0 = torch.rand(777, device=DEV)

    def build():
        ps = _clone(ps0)
        opts = _opts(ps, SparseAdam)
        extra = torch.nn.Parameter(extra0.clone())
        opts["extra"] = Adam([extra], lr=1e-3, eps=1e-15)
        return ps, extra, opts

    pa, ea, oa = build()
    pb, eb, ob = build()
    calls = []
    real_call = _backend.call

    def recording_call(name, *a, **kw):
        calls.append(name)
        return real_call(name, *a, **kw)

    for step, share in enumerate((True, False, "two lists")):
        ids = _ids(n, 600, rng)
        if share == "two lists":
            _set_grads((pa, pb), _ids(n, 333, rng), 20 + step, keys=("means", "quats"))
            _set_grads((pa, pb), ids, 30 + step, keys=("scales", "opacities", "sh0", "shN"))
        else:
            _set_grads((pa, pb), ids, 20 + step, share=share)
        for e in (ea, eb):
            e.grad = torch.full_like(e, 0.25 * (step + 1))
        assert S.B is _backend
        _backend.call = recording_call
        try:
            del calls[:]
            step_all(oa)
        finally:
            _backend.call = real_call
        assert all(p.grad is None for p in pa.values()) and ea.grad is None
        want = {True: (1, 1), False: (6, 6), "two lists": (2, 2)}[share]
        assert (calls.count("gs_sort_pairs_u64_i32"), calls.count("gs_sparse_adam_multi")) == want, calls
        assert calls.count("gs_adam_multi") == 1
        for o in ob.values():
            o.step()
    torch.cuda.synchronize()
    for k in pa:
        sa, sb = oa[k].state[pa[k]], ob[k].state[pb[k]]
        assert sa["step"] == sb["step"] == 3
        for a, b in ((pa[k].detach(), pb[k].detach()), (sa["exp_avg"], sb["exp_avg"]), (sa["exp_avg_sq"], sb["exp_avg_sq"])):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k
        assert not torch.equal(pa[k].detach(), ps0[k].detach())
    assert torch.equal(ea.detach().view(torch.int32), eb.detach().view(torch.int32)) and not torch.equal(ea.detach(), extra0)
    assert float(oa["extra"].state[ea]["step"]) == 3.0


def test_sparse_step_after_densification():
    """strategy.ops.duplicate appends rows to every parameter and zero rows to its optimizer state; the next sparse step, whose
    indices reach into the new rows, still agrees with torch's."""
    from gscodec_studio_amd.optimizers import SparseAdam, step_all
    from gscodec_studio_amd.strategy import ops

    n, rng = 500, np.random.default_rng(8)
    ps0 = _params(n, seed=2)
    pa, pb = torch.nn.ParameterDict(_clone(ps0)), torch.nn.ParameterDict(_clone(ps0))
    oa, ob = _opts(pa, SparseAdam), _opts(pb, torch.optim.SparseAdam)
    _set_grads((pa, pb), _ids(n, 300, rng), 1)
    step_all(oa)
    for o in ob.values():
        o.step()
        o.zero_grad(set_to_none=True)
    mask = torch.from_numpy(rng.random(n) < 0.2).to(DEV)
    ops.duplicate(pa, oa, {}, mask)
    ops.duplicate(pb, ob, {}, mask)
    n2 = pa["means"].shape[0]
    assert n2 == n + int(mask.sum()) > n
    ids = torch.cat([_ids(n2 - 1, 400, rng), torch.tensor([n2 - 1], device=DEV)])  # old and new rows, the last one among them
    assert int((ids >= n).sum()) > 1
    _set_grads((pa, pb), ids, 2)
    step_all(oa)
    for o in ob.values():
        o.step()
    torch.cuda.synchronize()
    _compare(oa, ob, pa, pb, "after duplicate")
    assert oa["shN"].state[pa["shN"]]["exp_avg"].shape == (n2, 15, 3) and oa["shN"].state[pa["shN"]]["step"] == 2


def test_packed_sparse_grad_render_end_to_end():
    """rasterization(packed=True, sparse_grad=True), 2 cameras, 2,000 splats, 64 x 48, one backward; sparsify_grads, step_all;
    the same gradients, cloned, through torch.optim.SparseAdam.  Every splat absent from gaussian_ids keeps its bits."""
    import gscodec_studio_amd as G
    from gscodec_studio_amd.optimizers import SparseAdam, sparsify_grads, step_all

    n, C, W, H = 2000, 2, 64, 48
    g = garden(n, scale_mult=2.0)
    assert g["means"].shape[0] == n
    sh = torch.rand(n, 16, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    pa = torch.nn.ParameterDict({"means": torch.nn.Parameter(T(g["means"])), "scales": torch.nn.Parameter(T(g["scales"]).log()),
                                 "quats": torch.nn.Parameter(T(g["quats"])), "opacities": torch.nn.Parameter(torch.logit(T(g["opacities"]).clamp(0.01, 0.99))),
                                 "sh0": torch.nn.Parameter(sh[:, :1].clone()), "shN": torch.nn.Parameter(sh[:, 1:].clone() * 0.1)})
    Ks = g["Ks"][:C].copy()
    Ks[:, 0] *= W / g["width"]
    Ks[:, 1] *= H / g["height"]
    rc, ra, info = G.rasterization(pa["means"], pa["quats"], torch.exp(pa["scales"]), torch.sigmoid(pa["opacities"]),
                                   torch.cat([pa["sh0"], pa["shN"]], 1), T(g["viewmats"][:C]), T(Ks), W, H, sh_degree=3, packed=True,
                                   sparse_grad=True)
    weights = torch.rand(rc.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    ((rc * weights).sum() + 0.5 * ra.sum()).backward()
    gids = info["gaussian_ids"]
    assert 0 < gids.unique().numel() < n and gids.numel() > gids.unique().numel()  # some splats unseen, some seen by both cameras
    # (quats: the projection backward's COO as it is; means: made dense by the SH view directions' share; shN: dense)
    assert pa["quats"].grad.is_sparse and pa["quats"].grad._indices().data_ptr() == gids.data_ptr() and not pa["shN"].grad.is_sparse
    sparsify_grads(pa, gids, coalesced=False)
    assert all(p.grad.is_sparse for p in pa.values())
    pb = _clone(pa)
    for k in pa:
        gr = pa[k].grad
        pb[k].grad = torch.sparse_coo_tensor(gr._indices().clone(), gr._values().clone(), gr.shape, is_coalesced=gr.is_coalesced())
    first = {k: p.detach().clone() for k, p in pa.items()}
    oa, ob = _opts(pa, SparseAdam), _opts(pb, torch.optim.SparseAdam)
    step_all(oa)
    for o in ob.values():
        o.step()
    torch.cuda.synchronize()
    _compare(oa, ob, pa, pb, "packed sparse_grad render")
    unseen = torch.ones(n, dtype=torch.bool, device=DEV)
    unseen[gids] = False
    for k in pa:
        st = oa[k].state[pa[k]]
        assert torch.equal(pa[k].detach()[unseen].view(torch.int32), first[k][unseen].view(torch.int32)), k
        assert not bool(st["exp_avg"][unseen].any()) and not bool(st["exp_avg_sq"][unseen].any()), k
        assert torch.equal(st["exp_avg"][unseen].view(torch.int32), torch.zeros_like(st["exp_avg"][unseen]).view(torch.int32)), k
        assert not torch.equal(pa[k].detach()[~unseen], first[k][~unseen]), k
