"""gscodec_studio_amd.optimizers on the GPU (gs_adam_multi): dense Adam against torch.optim.Adam (single-tensor and foreach),
SelectiveAdam against a float32 restatement of the reference kernel (gsplat/cuda/csrc/adam.cu:31-40) with the invisible rows
bit-identical, step_all batching, state_dict compatibility with torch.optim.Adam and a densification-style parameter
replacement, and a few training iterations of the trainer's loop against step_all."""
import copy

import numpy as np
import pytest
import torch

from util import garden

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
N = 100_003  # odd: tails and n % 4 != 0 in every tensor
SHAPES = {"means": (N, 3), "quats": (N, 4), "scales": (N, 3), "opacities": (N,), "sh0": (N, 1, 3), "shN": (N, 15, 3)}
LRS = {"means": 1.6e-3, "quats": 1e-3, "scales": 5e-3, "opacities": 5e-2, "sh0": 2.5e-3, "shN": 2.5e-3 / 20}


def _params(seed=0, misaligned=True):
    g = torch.Generator(device=DEV).manual_seed(seed)
    ps = {k: torch.nn.Parameter(torch.randn(s, device=DEV, generator=g)) for k, s in SHAPES.items()}
    if misaligned:  # 4 bytes past a 16-byte boundary: p and its grad / moments have different offsets -> the scalar path
        base = torch.randn(N + 1, device=DEV, generator=g)
        ps["misaligned"] = torch.nn.Parameter(base[1:])
        assert ps["misaligned"].data_ptr() % 16 == 4
    return ps


def _clone(ps):
    return {k: torch.nn.Parameter(v.detach().clone()) for k, v in ps.items()}


def _set_grads(ps, step, seed=1):
    g = torch.Generator(device=DEV).manual_seed(seed * 1000 + step)
    for i, (k, p) in enumerate(ps.items()):
        p.grad = torch.randn(p.shape, device=DEV, generator=g) * (0.1 * (i + 1))


def _ulp(a, b):
    """Largest distance in float32 ulps over the elements with |b| >= 2^-10 (next to zero an ulp count says nothing)."""
    keep = b.abs() >= 2.0 ** -10
    a, b = a[keep], b[keep]
    ai, bi = a.contiguous().view(torch.int32).long(), b.contiguous().view(torch.int32).long()
    ai = torch.where(ai < 0, -(ai & 0x7FFFFFFF), ai)
    bi = torch.where(bi < 0, -(bi & 0x7FFFFFFF), bi)
    return int((ai - bi).abs().max()) if ai.numel() else 0


def _assert_state_close(ours, ref, p_ours, p_ref, rtol=1e-6, p_atol=1e-7):
    torch.testing.assert_close(p_ours.detach(), p_ref.detach(), rtol=rtol, atol=p_atol)
    so, sr = ours.state[p_ours], ref.state[p_ref]
    torch.testing.assert_close(so["exp_avg"], sr["exp_avg"], rtol=rtol, atol=1e-6)
    torch.testing.assert_close(so["exp_avg_sq"], sr["exp_avg_sq"], rtol=rtol, atol=1e-9)
    assert so["step"].device.type == "cpu" and so["step"].dtype == torch.float32 and float(so["step"]) == float(sr["step"])
    return max(_ulp(p_ours.detach(), p_ref.detach()), _ulp(so["exp_avg"], sr["exp_avg"]), _ulp(so["exp_avg_sq"], sr["exp_avg_sq"]))


def _per_param_opts(ps, cls, **kw):
    return {k: cls([{"params": [p], "lr": LRS.get(k, 1e-3), "name": k}], eps=1e-15, betas=(0.9, 0.999), **kw) for k, p in ps.items()}


def test_dense_adam_matches_torch():
    """optimizers.Adam against torch.optim.Adam(foreach=False) and (foreach=True), 20 steps, an ExponentialLR on the means.
    torch's kernels contract some of Adam's multiply-adds into fmas, this kernel rounds every operation: the two differ in the
    last bits, as torch's two paths do between themselves.  A parameter that crosses zero has no relative bound, so p also gets
    an absolute slack of 4 float32 ulps of each step's size (lr), summed over the steps."""
    from gscodec_studio_amd.optimizers import Adam

    steps = 20
    ps0 = _params()
    pa, ps_, pf = _clone(ps0), _clone(ps0), _clone(ps0)
    pa["misaligned"] = torch.nn.Parameter(torch.empty(N + 1, device=DEV)[1:].copy_(ps0["misaligned"].detach()))
    assert pa["misaligned"].data_ptr() % 16 == 4
    oa, os_, of = _per_param_opts(pa, Adam), _per_param_opts(ps_, torch.optim.Adam, foreach=False), _per_param_opts(pf, torch.optim.Adam, foreach=True)
    scheds = [torch.optim.lr_scheduler.ExponentialLR(o["means"], gamma=0.9) for o in (oa, os_, of)]
    for step in range(steps):
        for ps, opts in ((pa, oa), (ps_, os_), (pf, of)):
            _set_grads(ps, step)
            for o in opts.values():
                o.step()
        for s in scheds:
            s.step()
    torch.cuda.synchronize()
    worst = {"single": 0, "foreach": 0, "torch single vs foreach": 0}
    for k in pa:
        slack = steps * LRS.get(k, 1e-3) * 4 * 2.0 ** -23
        worst["single"] = max(worst["single"], _assert_state_close(oa[k], os_[k], pa[k], ps_[k], p_atol=slack))
        worst["foreach"] = max(worst["foreach"], _assert_state_close(oa[k], of[k], pa[k], pf[k], p_atol=slack))
        sf, ss = of[k].state[pf[k]], os_[k].state[ps_[k]]  # (for scale only: torch's two paths against each other)
        worst["torch single vs foreach"] = max(worst["torch single vs foreach"], _ulp(pf[k].detach(), ps_[k].detach()),
                                               _ulp(sf["exp_avg"], ss["exp_avg"]), _ulp(sf["exp_avg_sq"], ss["exp_avg_sq"]))
    assert oa["means"].param_groups[0]["lr"] == os_["means"].param_groups[0]["lr"] < LRS["means"]
    print(f"[dense adam, {steps} steps] largest ULP distance over p / exp_avg / exp_avg_sq: {worst}")


def _selective_ref(p, g, m, v, vis, lr, b1, b2, eps, M):
    """adam.cu:31-40 restated in float32 torch ops (one rounding per operation), applied where vis[e // M] is set."""
    f = np.float32
    w1, w2 = float(f(1) - f(b1)), float(f(1) - f(b2))
    b1, b2, nlr, eps = float(f(b1)), float(f(b2)), float(-f(lr)), float(f(eps))
    n = vis.numel() * M
    pv, gv, mv, vv = (t.reshape(-1)[:n] for t in (p, g, m, v))
    m_new = mv * b1 + gv * w1
    v_new = vv * b2 + (gv * w2) * gv
    p_new = pv + (m_new * nlr) / (torch.sqrt(v_new) + eps)
    keep = vis.bool().repeat_interleave(M)
    return [torch.where(keep, a, b) for a, b in ((p_new, pv), (m_new, mv), (v_new, vv))]


def _bits(t):
    return t.detach().contiguous().view(torch.int32).clone()


def test_selective_adam_matches_reference_and_leaves_invisible_rows_alone():
    from gscodec_studio_amd._c_adapter import _C
    from gscodec_studio_amd.optimizers import SelectiveAdam

    ps = _params(seed=3, misaligned=False)
    g = torch.Generator(device=DEV).manual_seed(7)
    vis = torch.rand(N, device=DEV, generator=g) < 0.25
    opts = _per_param_opts(ps, SelectiveAdam)
    for step in range(3):
        _set_grads(ps, step, seed=3)
        if step == 0:
            for k, p in ps.items():  # non-zero moments from the start, so an invisible row that was written would show
                opts[k].state[p]["step"] = torch.tensor(0.0)
                opts[k].state[p]["exp_avg"] = torch.randn(p.shape, device=DEV, generator=g)
                opts[k].state[p]["exp_avg_sq"] = torch.rand(p.shape, device=DEV, generator=g)
        before = {k: (p.detach().clone(), opts[k].state[p]["exp_avg"].clone(), opts[k].state[p]["exp_avg_sq"].clone()) for k, p in ps.items()}
        for k in ps:
            opts[k].step(vis)
        torch.cuda.synchronize()
        for k, p in ps.items():
            M = p.numel() // N
            st = opts[k].state[p]
            grp = opts[k].param_groups[0]
            want = _selective_ref(before[k][0], p.grad, before[k][1], before[k][2], vis, grp["lr"], *grp["betas"], grp["eps"], M)
            got = [p.detach().reshape(-1), st["exp_avg"].reshape(-1), st["exp_avg_sq"].reshape(-1)]
            rows = vis.repeat_interleave(M)
            for w, gt, b in zip(want, got, before[k]):
                torch.testing.assert_close(gt[rows], w[rows], rtol=1e-6, atol=1e-7)
                assert torch.equal(_bits(gt[~rows]), _bits(b.reshape(-1)[~rows])), f"{k}: an invisible row changed"
            assert float(st["step"]) == 0.0  # the reference never advances it

    # the reference's positional entry point, on buffers 4 bytes past a 16-byte boundary (head + quads + tail)
    p = ps["shN"]
    M = p.numel() // N
    st = opts["shN"].state[p]
    grp = opts["shN"].param_groups[0]
    args = [p.detach(), p.grad, st["exp_avg"], st["exp_avg_sq"]]
    aligned = [a.clone() for a in args]
    shifted = [torch.empty(a.numel() + 1, device=DEV)[1:].copy_(a.reshape(-1)) for a in args]
    for bufs in (aligned, shifted):
        _C.selective_adam_update(bufs[0], bufs[1], bufs[2], bufs[3], vis, grp["lr"], grp["betas"][0], grp["betas"][1], grp["eps"], N, M)
    want = _selective_ref(args[0], args[1], args[2], args[3], vis, grp["lr"], *grp["betas"], grp["eps"], M)
    torch.cuda.synchronize()
    for i in (0, 2, 3):
        assert torch.equal(_bits(aligned[i]).reshape(-1), _bits(shifted[i])), "aligned and shifted buffers differ"
    for w, i in zip(want, (0, 2, 3)):
        torch.testing.assert_close(aligned[i].reshape(-1), w, rtol=1e-6, atol=1e-7)


def _unused():
    return torch.nn.Parameter(torch.randn(N, 2, device=DEV, generator=torch.Generator(device=DEV).manual_seed(6)))


def _batch_run():
    from gscodec_studio_amd.optimizers import Adam, step_all

    ps = _params(seed=5)
    del ps["misaligned"]
    ps["unused"] = _unused()
    opts = {}
    for i, (k, p) in enumerate(ps.items()):
        cls = torch.optim.Adam if i % 2 else Adam
        opts[k] = cls([{"params": [p], "lr": LRS.get(k, 1e-3), "name": k}], eps=1e-15, betas=(0.9, 0.999))
    for step in range(4):
        _set_grads(ps, step, seed=5)
        ps["unused"].grad = None
        step_all(opts)
        assert all(p.grad is None for p in ps.values())
    torch.cuda.synchronize()
    return ps, opts


def test_step_all_batches_bit_identically():
    from gscodec_studio_amd.optimizers import Adam

    ps, opts = _batch_run()
    ps2, opts2 = _batch_run()
    ref = _params(seed=5)
    del ref["misaligned"]
    ref["unused"] = _unused()
    # the same sequence, each optimizer stepped on its own through optimizers.Adam
    ro = {k: Adam([{"params": [p], "lr": LRS.get(k, 1e-3), "name": k}], eps=1e-15, betas=(0.9, 0.999)) for k, p in ref.items()}
    for step in range(4):
        _set_grads(ref, step, seed=5)
        ref["unused"].grad = None
        for o in ro.values():
            o.step()
            o.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    for k in ps:
        assert torch.equal(_bits(ps[k]), _bits(ps2[k])), f"{k}: two runs differ"
        if k == "unused":
            assert len(opts[k].state) == 0 and torch.equal(ps[k].detach(), ref[k].detach())
            continue
        assert torch.equal(_bits(ps[k]), _bits(ref[k])), f"{k}: step_all differs from optimizers.Adam"
        for s in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(_bits(opts[k].state[ps[k]][s]), _bits(ro[k].state[ref[k]][s])), (k, s)
        assert float(opts[k].state[ps[k]]["step"]) == 4.0


def test_state_dict_round_trips_and_densification():
    from gscodec_studio_amd.compression import reorder_splats
    from gscodec_studio_amd.optimizers import Adam

    for first, second in ((torch.optim.Adam, Adam), (Adam, torch.optim.Adam)):
        ps = _params(seed=9, misaligned=False)
        o1 = _per_param_opts(ps, first)
        for step in range(3):
            _set_grads(ps, step, seed=9)
            for o in o1.values():
                o.step()
        sd = {k: copy.deepcopy(o.state_dict()) for k, o in o1.items()}
        pb = _clone(ps)
        o2 = _per_param_opts(pb, second)
        for k in o2:
            o2[k].load_state_dict(sd[k])
        for step in range(3, 6):
            _set_grads(ps, step, seed=9)
            _set_grads(pb, step, seed=9)
            for k in ps:
                o1[k].step()
                o2[k].step()
        torch.cuda.synchronize()
        for k in ps:
            _assert_state_close(o2[k], o1[k], pb[k], ps[k])

    # densification (strategy/ops.py: cat rows, zeros for the new moments, "step" kept), then reorder_splats, then steps
    runs = []
    for cls in (torch.optim.Adam, Adam):
        ps = _params(seed=11, misaligned=False)
        opts = _per_param_opts(ps, cls)
        _set_grads(ps, 0, seed=11)
        for o in opts.values():
            o.step()
        sel = torch.arange(0, N, 7, device=DEV)
        for k in list(ps):
            old = ps[k]
            new = torch.nn.Parameter(torch.cat([old.detach(), old.detach()[sel]]))
            st = opts[k].state.pop(old)
            for key in ("exp_avg", "exp_avg_sq"):
                st[key] = torch.cat([st[key], torch.zeros_like(st[key][sel])])
            opts[k].param_groups[0]["params"] = [new]
            opts[k].state[new] = st
            ps[k] = new
        perm = torch.randperm(ps["means"].shape[0], device=DEV, generator=torch.Generator(device=DEV).manual_seed(0))
        reorder_splats(ps, opts, perm=perm)
        for step in range(1, 4):
            _set_grads(ps, step, seed=11)
            for o in opts.values():
                o.step()
        torch.cuda.synchronize()
        runs.append((ps, opts))
    (pt, ot), (pa, oa) = runs
    for k in pt:
        _assert_state_close(oa[k], ot[k], pa[k], pt[k])


def _trainer_scene(n=4000):
    fx = garden(n)
    rs = np.random.RandomState(0)
    T = lambda a: torch.tensor(np.asarray(a, np.float32), device=DEV)  # noqa: E731
    sh = np.zeros((n, 16, 3), np.float32)
    sh[:, 0] = (fx["rgb"] - 0.5) / 0.2820947917738781
    sh[:, 1:] = rs.randn(n, 15, 3).astype(np.float32) * 0.05
    params = {"means": T(fx["means"]), "quats": T(fx["quats"]), "scales": T(np.log(fx["scales"] * 4 + 1e-4)),
              "opacities": T(rs.uniform(-2, 3, n)), "sh0": T(sh[:, :1]), "shN": T(sh[:, 1:])}
    cams = {"viewmats": T(fx["viewmats"][:2]), "Ks": T(fx["Ks"][:2]), "W": fx["width"], "H": fx["height"]}
    return params, cams


def _render(ps, cams, packed=False):
    from gscodec_studio_amd import rasterization

    rc, ra, meta = rasterization(ps["means"], ps["quats"], torch.exp(ps["scales"]), torch.sigmoid(ps["opacities"]),
                                 torch.cat([ps["sh0"], ps["shN"]], 1), cams["viewmats"], cams["Ks"], cams["W"], cams["H"], sh_degree=3,
                                 packed=packed, deterministic=True)
    return rc, ra, meta


@pytest.mark.parametrize("visible_adam", [False, True])
def test_trainer_loop_against_step_all(visible_adam):
    from gscodec_studio_amd.optimizers import SelectiveAdam, step_all, visibility_mask

    init, cams = _trainer_scene()
    target = torch.rand(cams["viewmats"].shape[0], cams["H"], cams["W"], 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    finals = []
    for use_step_all in (False, True):
        ps = {k: torch.nn.Parameter(v.clone()) for k, v in init.items()}
        cls = SelectiveAdam if visible_adam else torch.optim.Adam
        opts = {k: cls([{"params": [p], "lr": LRS[k], "name": k}], eps=1e-15, betas=(0.9, 0.999)) for k, p in ps.items()}
        for it in range(3):
            rc, _, meta = _render(ps, cams)
            loss = (rc - target).abs().mean()
            loss.backward()
            ref_mask = (meta["radii"] > 0).any(0)
            if use_step_all:
                vis = visibility_mask(meta, init["means"].shape[0]) if visible_adam else None
                if visible_adam:
                    assert torch.equal(vis, ref_mask)
                step_all(opts, visibility=vis)
            elif visible_adam:  # the reference kernel restated in torch, per optimizer (the trainer's loop with SelectiveAdam)
                with torch.no_grad():
                    for k, p in ps.items():
                        st = opts[k].state.setdefault(p, {})
                        if not st:
                            st.update(step=torch.tensor(0.0), exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p))
                        M = p.numel() // ref_mask.numel()
                        np_, nm, nv = _selective_ref(p.detach(), p.grad, st["exp_avg"], st["exp_avg_sq"], ref_mask, LRS[k], 0.9, 0.999,
                                                     1e-15, M)
                        p.copy_(np_.view_as(p))
                        st["exp_avg"].copy_(nm.view_as(p))
                        st["exp_avg_sq"].copy_(nv.view_as(p))
                        opts[k].zero_grad(set_to_none=True)
            else:
                for o in opts.values():
                    o.step()
                    o.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        finals.append({k: p.detach().clone() for k, p in ps.items()})
    for k in init:
        torch.testing.assert_close(finals[1][k], finals[0][k], rtol=1e-5, atol=1e-6)

    if visible_adam:  # the packed meta: gaussian_ids scattered, as simple_trainer.py does
        ps = {k: v.clone() for k, v in init.items()}
        _, _, meta = _render(ps, cams, packed=True)
        want = torch.zeros(init["means"].shape[0], dtype=torch.bool, device=DEV)
        want.scatter_(0, meta["gaussian_ids"], True)
        assert torch.equal(visibility_mask(meta, init["means"].shape[0]), want)
