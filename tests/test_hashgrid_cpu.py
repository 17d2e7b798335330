"""CPU: host side of the hash-grid Gaussian entropy model -- module layout (state-dict keys, shapes, level offsets),
HashGridCompressionSimulation's models / optimizers / schedulers, bounding box and sampling against direct torch calls, the
refusals, and the float64 restatement's own consistency (tests/hashgrid_reference.py).  No kernel is launched here."""
import copy

import pytest
import torch

import hashgrid_reference as HR

RES_3D = (18, 24, 33, 44, 59, 80, 108, 148, 201, 275, 376, 514)
RES_2D = (130, 258, 514, 1026)
STEPS = {"means": -1, "scales": 10, "quats": 20, "opacities": -1, "sh0": 30, "shN": -1}


def expected_offsets(res, D, log2):
    off = [0]
    for r in res:
        off.append(off[-1] + -(-min(2 ** log2, r ** D) // 8) * 8)
    return off


@pytest.mark.parametrize("channel", [3, 4])
def test_entropy_gaussian_state_dict(channel):
    from gscodec_studio_amd.compression_simulation import Entropy_gaussian

    m = Entropy_gaussian(channel)
    sd = m.state_dict()
    keys = ["likelihood_lower_bound.bound"]
    for g in ("xyz", "xy", "xz", "yz"):
        keys += [f"param_regressor.hash_grid.encoding_{g}.{k}" for k in ("params", "offsets_list", "resolutions_list")]
    keys += [f"param_regressor.mlp_regressor.{i}.{k}" for i in (0, 2) for k in ("weight", "bias")]
    assert list(sd) == keys
    hg = m.param_regressor.hash_grid
    assert hg.output_dim == 48
    assert tuple(sd["param_regressor.hash_grid.encoding_xyz.params"].shape) == (95_944, 2)
    for g in ("xy", "xz", "yz"):
        assert tuple(sd[f"param_regressor.hash_grid.encoding_{g}.params"].shape) == (115_208, 2)
    assert hg.encoding_xyz.offsets_list.tolist() == expected_offsets(RES_3D, 3, 13)
    assert hg.encoding_xy.offsets_list.tolist() == expected_offsets(RES_2D, 2, 15)
    assert hg.encoding_xyz.offsets_list.dtype == torch.int32 and hg.encoding_xyz.resolutions_list.dtype == torch.int32
    assert hg.encoding_xyz.resolutions_list.tolist() == list(RES_3D) and hg.encoding_yz.resolutions_list.tolist() == list(RES_2D)
    assert tuple(sd["param_regressor.mlp_regressor.0.weight"].shape) == (channel * 5, 48)
    assert tuple(sd["param_regressor.mlp_regressor.2.weight"].shape) == (channel * 2, channel * 5)
    assert float(sd["likelihood_lower_bound.bound"]) == pytest.approx(1e-6)
    p = hg.encoding_xz.params.detach()
    assert float(p.abs().max()) <= 1e-4 and float(p.std()) > 2e-5  # uniform_(-1e-4, 1e-4)
    # bound_min / bound_max stay out of the state dict and follow the module
    assert float(m.param_regressor.bound_min[0, 0]) == -100 and float(m.param_regressor.bound_max[0, 2]) == 100
    assert m.double().param_regressor.bound_max.dtype == torch.float64
    m2 = Entropy_gaussian(channel)
    m2.load_state_dict(copy.deepcopy(sd), strict=True)
    assert torch.equal(m2.param_regressor.hash_grid.encoding_xy.params, hg.encoding_xy.params.float())


def test_grid_encoder_defaults_and_level_rows():
    from gscodec_studio_amd.compression_simulation import GridEncoder

    e = GridEncoder()
    assert (e.num_dim, e.n_features, e.n_levels, e.log2_hashmap_size, e.output_dim, e.n_output_dims) == (3, 2, 12, 19, 24, 24)
    assert e.ste_binary and not e.ste_multistep and not e.add_noise and e.Q == 1
    assert e.offsets_list.tolist() == expected_offsets((16, 23, 32, 46, 64, 92, 128, 184, 256, 368, 512, 736), 3, 19)
    small = GridEncoder(num_dim=2, n_features=4, resolutions_list=(6, 10, 34), log2_hashmap_size=6)
    assert small.offsets_list.tolist() == [0, 40, 104, 168] and tuple(small.params.shape) == (168, 4)
    for bad in (dict(num_dim=1), dict(n_features=3), dict(resolutions_list=tuple(range(3, 36)))):
        with pytest.raises(NotImplementedError):
            GridEncoder(**bad)


def test_ste_functions_on_cpu():
    from gscodec_studio_amd.compression_simulation import STE_binary, STE_multistep

    p = torch.tensor([-1.5, -1.0, -0.0, 0.0, 1.0, 1.5, float("nan")], requires_grad=True)
    out = STE_binary.apply(p)
    assert out.tolist() == [-1, -1, 1, 1, 1, 1, 0]
    out.sum().backward()
    assert p.grad.tolist() == [0, 1, 1, 1, 1, 0, 0]
    assert torch.equal(HR.embed(p.detach(), True).float(), out.detach()) and torch.equal(HR.ste_mask(p.detach(), True).float(), p.grad)
    x = torch.tensor([0.26, -0.74, 1.1], requires_grad=True)
    q = STE_multistep.apply(x, 0.5)
    assert q.tolist() == [0.5, -0.5, 1.0]
    q.sum().backward()
    assert x.grad.tolist() == [1, 1, 1]


def test_simulation_models_optimizers_schedulers():
    from gscodec_studio_amd.compression_simulation import Entropy_gaussian, HashGridCompressionSimulation

    sim = HashGridCompressionSimulation(entropy_model_enable=True, entropy_steps=STEPS, device="cpu")
    assert sim.entropy_model_type == "gaussian_model" and sim.entropy_min_step == 10
    assert {k: type(v) for k, v in sim.entropy_models.items()} == {
        "means": type(None), "scales": Entropy_gaussian, "quats": Entropy_gaussian, "opacities": type(None),
        "sh0": Entropy_gaussian, "shN": type(None)}
    assert [sim.entropy_models[k].param_regressor.channel for k in ("scales", "quats", "sh0")] == [3, 4, 3]
    for k in ("scales", "quats", "sh0"):
        opt, sch = sim.entropy_model_optimizers[k], sim.entropy_model_schedulers[k]
        assert isinstance(opt, torch.optim.Adam)
        assert [(g["name"], g["lr"], len(g["params"])) for g in opt.param_groups] == [("hash_grid", 5e-3, 4), ("mlp_regressor", 5e-3, 4)]
        assert isinstance(sch, torch.optim.lr_scheduler.ExponentialLR)
        assert sch.gamma == pytest.approx(0.01 ** (1.0 / (30000 - STEPS[k])), rel=1e-12)
    for k in ("means", "opacities", "shN"):
        assert sim.entropy_model_optimizers[k] is None and sim.entropy_model_schedulers[k] is None
    assert sim.entropy_model_option == {"means": False, "scales": True, "quats": True, "opacities": False, "sh0": True, "shN": False}
    off = HashGridCompressionSimulation(entropy_model_enable=True, entropy_steps=dict(STEPS, quats=-1), device="cpu")
    assert off.entropy_model_option["quats"] is False and off.entropy_min_step == 10
    plain = HashGridCompressionSimulation()
    assert plain.entropy_model_enable is False and plain.entropy_model_type == "gaussian_model"
    with pytest.raises(TypeError):  # the base class's arguments except entropy_model_type
        HashGridCompressionSimulation(entropy_model_type="factorized_model")


def test_bbox_and_sampling_follow_the_direct_torch_calls():
    from gscodec_studio_amd.compression_simulation import HashGridCompressionSimulation

    sim = HashGridCompressionSimulation(entropy_model_enable=True, entropy_steps=STEPS, device="cpu")
    g = torch.Generator().manual_seed(3)
    pos = torch.randn(5000, 3, generator=g) * torch.tensor([1.0, 2.0, 0.5])
    sim._estiblish_bbox(pos)
    lo, hi = torch.quantile(pos, torch.tensor([0.01, 0.99]), dim=0)
    assert torch.equal(sim.bbox_lower_bound, lo) and torch.equal(sim.bbox_upper_bound, hi)
    inside = sim._get_pts_inside_bbox(pos)
    assert torch.equal(inside, torch.all((pos >= lo) & (pos <= hi), dim=1)) and 0.9 < float(inside.float().mean()) < 0.99
    torch.manual_seed(11)
    mask = sim._random_sample_pts(inside)
    torch.manual_seed(11)
    r = torch.rand_like(inside.float())
    r[~inside] = 0
    want = r >= torch.quantile(r[inside], 1 - 0.05)
    assert torch.equal(mask, want) and not bool((mask & ~inside).any())
    assert abs(int(mask.sum()) - 0.05 * int(inside.sum())) <= 2
    torch.manual_seed(11)
    assert int(sim._random_sample_pts(inside, ratio=0.5).sum()) > 5 * int(mask.sum())


def splats_cpu(n=64):
    g = torch.Generator().manual_seed(0)
    return {"means": torch.randn(n, 3, generator=g), "scales": torch.randn(n, 3, generator=g), "quats": torch.randn(n, 4, generator=g),
            "opacities": torch.randn(n, generator=g), "sh0": torch.rand(n, 1, 3, generator=g), "shN": torch.randn(n, 15, 3, generator=g)}


def test_refusals():
    from gscodec_studio_amd.compression_simulation import (CompressionSimulation, Entropy_gaussian, GridEncoder,
                                                           HashGridCompressionSimulation, mix_3D2D_encoding)

    with pytest.raises(NotImplementedError, match="HashGridCompressionSimulation"):  # the old route stays closed
        CompressionSimulation(entropy_model_enable=True, entropy_model_type="gaussian_model", entropy_steps=STEPS, device="cpu")
    sim = HashGridCompressionSimulation(entropy_model_enable=True, entropy_steps=STEPS, device="cpu")
    with pytest.raises(RuntimeError, match="_estiblish_bbox"):
        sim.simulate_compression(splats_cpu(), step=11)
    # a forward on CPU tensors raises, as everywhere in the package
    with pytest.raises(RuntimeError, match="no CPU"):
        Entropy_gaussian(3)(torch.zeros(5, 3), 0.05, pos=torch.zeros(5, 3))
    with pytest.raises(RuntimeError, match="no CPU"):
        GridEncoder(resolutions_list=(4, 6), log2_hashmap_size=7)(torch.rand(5, 3))
    with pytest.raises(RuntimeError, match="no CPU"):
        mix_3D2D_encoding(2, (4, 6), 7, (6, 10), 6, True, False, False, 1)(torch.rand(5, 3))
    with pytest.raises(NotImplementedError):
        GridEncoder(resolutions_list=(4, 6), log2_hashmap_size=7)(torch.rand(5, 3), binary_vxl=torch.ones(4, 4, 4, dtype=torch.bool))
    with pytest.raises(AssertionError):
        Entropy_gaussian(3)(torch.zeros(5, 3), 0.05)  # pos is required, as in the reference


# one 3-D grid of two levels (dense 4^3, hashed 6^3) over 4 points; pointers are filled in by the caller
ENC_BASE = dict(n=4, pos_dim=3, n_grids=1, F=2, ste=1, pos=4096, params=[4096], rows=[192], num_dim=[3], axes=[0], n_levels=[2],
                res=[4, 6], off=[0, 64, 192], out=4096, v_out=4096, v_params=[4096], v_pos=4096)
# (override, text of the rule it breaks): every validation rule of gs_hashgrid_encode_fwd / _bwd
BAD_ENCODE = [(dict(F=3), "n_features"), (dict(F=0), "n_features"), (dict(pos_dim=4), "pos_dim"), (dict(n_grids=0), "n_grids"),
              (dict(n_grids=5), "n_grids"), (dict(num_dim=[1]), "num_dim"), (dict(axes=[1]), "axes"), (dict(num_dim=[2], axes=[0]), "axes"),
              (dict(axes=[4]), "axes"), (dict(pos_dim=2, num_dim=[2], axes=[3]), "axes"), (dict(n_levels=[0]), "levels"),
              (dict(n_levels=[33], res=[4] * 33, off=list(range(0, 34 * 8, 8)), rows=[400]), "levels"), (dict(res=[2, 6]), "resolution"),
              (dict(res=[4, -6]), "resolution"), (dict(off=[0, 64, 64]), "ascending"), (dict(off=[0, 64, 32]), "ascending"),
              (dict(off=[-8, 64, 192]), "ascending"), (dict(rows=[184]), "past the table"), (dict(pos=None), "null pointer"),
              (dict(params=[None]), "null pointer"), (dict(params=[4100]), "aligned")]
BAD_ENCODE_FWD = [(dict(out=None), "null pointer"), (dict(out=4100), "aligned")]
BAD_ENCODE_BWD = [(dict(v_out=None), "null pointer"), (dict(v_out=4100), "aligned"), (dict(v_params=[4100]), "aligned")]


def abi_encode(a, bwd=False, stream=None):
    """gs_hashgrid_encode_fwd / _bwd with the arguments of ``a`` (keys of ENC_BASE; lists become host arrays)."""
    import ctypes

    from gscodec_studio_amd import _backend as B

    arr = lambda t, v: None if v is None else (t * len(v))(*v)  # noqa: E731
    head = (a["n"], a["pos_dim"], a["n_grids"], a["F"], a["ste"], a["pos"], arr(ctypes.c_void_p, a["params"]),
            arr(ctypes.c_uint64, a["rows"]), arr(ctypes.c_uint32, a["num_dim"]), arr(ctypes.c_uint32, a["axes"]),
            arr(ctypes.c_uint32, a["n_levels"]), arr(ctypes.c_int32, a["res"]), arr(ctypes.c_int32, a["off"]))
    if bwd:
        B.call("gs_hashgrid_encode_bwd", *head, a["v_out"], arr(ctypes.c_void_p, a["v_params"]), a["v_pos"], stream)
    else:
        B.call("gs_hashgrid_encode_fwd", *head, a["out"], stream)


def test_abi_validation_precedes_the_launch():
    """Status 1 with the rule's message for bad arguments (host-side checks: no GPU needed, the pointers are never followed)."""
    from gscodec_studio_amd import _backend as B

    for bwd, extra in ((False, BAD_ENCODE_FWD), (True, BAD_ENCODE_BWD)):
        for over, text in BAD_ENCODE + extra + [(dict(rows=None), "null pointer"), (dict(off=None), "null pointer")]:
            with pytest.raises(RuntimeError, match=rf"status 1.*{text}"):
                abi_encode(dict(ENC_BASE, **over), bwd)
    abi_encode(dict(ENC_BASE, n=0, pos=None, out=None))  # empty input: status 0
    for name, args in (("gs_gaussian_bits_fwd", (4, 0, 8, 8, 8, 1e-6, 8, None)), ("gs_gaussian_bits_fwd", (4, 33, 8, 8, 8, 1e-6, 8, None)),
                       ("gs_gaussian_bits_bwd", (4, 33, 8, 8, 8, 1e-6, 8, 8, 8, None))):
        with pytest.raises(RuntimeError, match=r"status 1.*channels must be in 1\.\.32"):
            B.call(name, *args)
    with pytest.raises(RuntimeError, match=r"status 1.*null pointer"):
        B.call("gs_gaussian_bits_fwd", 4, 3, 8, None, 8, 1e-6, 8, None)
    with pytest.raises(RuntimeError, match=r"status 1.*null pointer"):
        B.call("gs_gaussian_bits_bwd", 4, 3, 8, 8, 8, 1e-6, 8, 8, None, None)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement against itself


def small_grids(F=2, seed=0, scale=1.0):
    from gscodec_studio_amd.compression_simulation import GridEncoder

    g = torch.Generator().manual_seed(seed)
    grids = []
    for D, axes, res, log2 in ((3, (0, 1, 2), (4, 6, 10, 18), 7), (2, (0, 1), (6, 10, 34), 6), (2, (0, 2), (6, 10, 34), 6), (2, (1, 2), (6, 10, 34), 6)):
        e = GridEncoder(num_dim=D, n_features=F, resolutions_list=res, log2_hashmap_size=log2)
        grids.append(dict(params=scale * torch.randn(e.params.shape, generator=g), num_dim=D, axes=axes, resolutions=list(res),
                          offsets=e.offsets_list.tolist()))
    return grids


def test_small_grid_offsets_cross_the_dense_hash_switch():
    grids = small_grids()
    assert grids[0]["offsets"] == [0, 64, 192, 320, 448]  # 4^3 = 64 dense, 6^3 = 216 > 128: hashed from the second level on
    assert grids[1]["offsets"] == [0, 40, 104, 168]       # 6^2 = 36 -> 40 dense, 10^2 = 100 > 64: hashed
    c = [torch.tensor([1, 2]), torch.tensor([2, 1]), torch.tensor([1, 3])]
    assert HR._rows(c, 4, 64).tolist() == [1 + 2 * 4 + 16, 2 + 4 + 3 * 16]
    h = [(1 * 1) ^ ((2 * 2654435761) & 0xFFFFFFFF) ^ ((1 * 805459861) & 0xFFFFFFFF), (2 * 1) ^ (2654435761 & 0xFFFFFFFF) ^ ((3 * 805459861) & 0xFFFFFFFF)]
    assert HR._rows(c, 6, 128).tolist() == [v % 128 for v in h]
    assert HR._rows(c[:2], 6, 40).tolist() == [1 + 2 * 6, 2 + 6]


@pytest.mark.parametrize("ste", [True, False])
def test_restatement_input_gradient_is_autograd_on_interior_points(ste):
    """Where no corner of a point's cell is a border corner (wn = 1) the reference's dy_dx formula IS the derivative of the
    forward; near the border the two differ on purpose (renormalisation does not enter the formula)."""
    grids = small_grids(F=2, scale=0.7)
    g = torch.Generator().manual_seed(5)
    pos = torch.rand(400, 3, generator=g, dtype=torch.float64)
    border = HR.has_border_corner(pos, grids)
    assert 0.2 < float(border.float().mean()) < 0.98  # both kinds are present
    v_out = torch.randn(400, 13 * 2, generator=g, dtype=torch.float64)
    p = pos.clone().requires_grad_(True)
    (HR.encode(p, grids, ste) * v_out).sum().backward()
    _, v_pos = HR.encode_backward(pos, grids, v_out, ste)
    # interior in EVERY level: compare level by level instead, so that points interior in some levels count there
    col = 0
    checked = 0
    for grid in grids:
        for l in range(len(grid["resolutions"])):
            one = [dict(grid, resolutions=grid["resolutions"][l:l + 1], offsets=grid["offsets"][l:l + 2])]
            vo = v_out[:, col:col + 2]
            col += 2
            inner = ~HR.has_border_corner(pos, one)
            q = pos.clone().requires_grad_(True)
            (HR.encode(q, one, ste) * vo).sum().backward()
            _, vp = HR.encode_backward(pos, one, vo, ste)
            assert torch.allclose(vp[inner], q.grad[inner], rtol=1e-10, atol=1e-12)
            checked += int(inner.sum())
            if (~inner).any() and not ste:
                assert not torch.allclose(vp[~inner], q.grad[~inner], rtol=1e-3, atol=1e-6)
    assert checked > 400
    assert p.grad.shape == v_pos.shape


def test_restatement_table_gradient_is_autograd_through_the_ste():
    from gscodec_studio_amd.compression_simulation import STE_binary

    grids = small_grids(F=4, scale=0.9)  # |p| > 1 on ~27 % of the entries: the mask matters
    g = torch.Generator().manual_seed(6)
    pos = torch.rand(300, 3, generator=g)
    pos[0] = torch.tensor([0.5, -1e-3, 0.5])
    pos[1] = torch.tensor([float("nan"), 0.2, 0.3])
    v_out = torch.randn(300, 13 * 4, generator=g, dtype=torch.float64)
    params = [gr["params"].double().requires_grad_(True) for gr in grids]
    emb = [dict(gr, params=STE_binary.apply(p)) for gr, p in zip(grids, params)]
    out = HR.encode(pos, emb, ste_binary=False)
    assert torch.equal(out.detach(), HR.encode(pos, grids, ste_binary=True))
    # columns: xyz 0..15 | xy 16..27 | xz 28..39 | yz 40..51
    assert bool((out[0, 28:40] != 0).any()) and bool((out[0, :28] == 0).all()) and bool((out[0, 40:] == 0).all())  # xz survives y < 0
    assert bool((out[1, :40] == 0).all()) and bool((out[1, 40:] != 0).any())  # yz survives a NaN x
    (out * v_out).sum().backward()
    v_params, v_pos = HR.encode_backward(pos, grids, v_out, True)
    for p, v in zip(params, v_params):
        assert torch.allclose(p.grad, v, rtol=1e-12, atol=1e-14)
    assert float(v_pos[0, 1]) == 0.0 and float(v_pos[1, 0]) == 0.0 and bool(torch.isfinite(v_pos).all())


def bits_inputs(M=4096, C=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    mean = 0.5 * torch.randn(M, C, generator=g)
    scale = 0.3 * torch.randn(M, C, generator=g).abs() + 0.02
    scale[:min(50, M // 8)] = 1e-12  # the clamp at 1e-9 is hit
    x = mean + 2.5 * scale * torch.randn(M, C, generator=g)
    return x, torch.cat([mean, scale], 1), 12 / 255


def test_bits_inputs_cover_body_tail_clamp_and_bound():
    x, net, q = bits_inputs()
    ref = HR.gaussian_bits(x, net, q, v_bits=torch.ones(4096, 4))
    like = ref["like"]
    assert 0.8 < float((like >= 1e-4).double().mean()) < 0.92
    assert 0.03 < float((like < 1e-6).double().mean()) < 0.08
    assert float(((like - 1e-6).abs() <= 2e-7).double().mean()) <= 0.01
    assert bool((ref["v_net"][:50, 4:] == 0).all())  # the clamp's gate: no gradient to a raw scale below 1e-9
    assert bool(torch.isfinite(ref["v_x"]).all())
    f32 = HR.gaussian_bits(x, net, q, dtype=torch.float32)
    body = like >= 1e-4
    assert float((f32["bits"].double() - ref["bits"])[body].abs().max()) < 4e-3
