"""The densification strategies without a GPU: the public surface (names, fields, defaults), the schedule arithmetic, the sanity
checks, the argument validation of the three native entry points, and the refusal of CPU tensors."""
import dataclasses
import math

import pytest
import torch

from gscodec_studio_amd import _backend as B
from gscodec_studio_amd import strategy as S
from gscodec_studio_amd.strategy import DefaultStrategy, MCMCStrategy, Strategy
from gscodec_studio_amd.strategy import default as default_mod
from gscodec_studio_amd.strategy import mcmc as mcmc_mod
from gscodec_studio_amd.strategy import ops

# the reference's fields and defaults (gsplat/strategy/default.py:79-94, mcmc.py:49-55), as values
DEFAULT_FIELDS = [
    ("prune_opa", 0.005), ("grow_grad2d", 0.0002), ("grow_scale3d", 0.01), ("grow_scale2d", 0.05), ("prune_scale3d", 0.1),
    ("prune_scale2d", 0.15), ("refine_scale2d_stop_iter", 0), ("refine_start_iter", 500), ("refine_stop_iter", 15_000),
    ("reset_every", 3000), ("refine_every", 100), ("pause_refine_after_reset", 0), ("absgrad", False), ("revised_opacity", False),
    ("verbose", False), ("key_for_gradient", "means2d"),
]
MCMC_FIELDS = [
    ("cap_max", 1_000_000), ("noise_lr", 5e5), ("refine_start_iter", 500), ("refine_stop_iter", 25_000), ("refine_every", 100),
    ("min_opacity", 0.005), ("verbose", False),
]


def _fields(cls):
    return [(f.name, f.default) for f in dataclasses.fields(cls)]


def test_public_surface_and_defaults():
    assert set(S.__all__) == {"Strategy", "DefaultStrategy", "MCMCStrategy"}
    assert issubclass(DefaultStrategy, Strategy) and issubclass(MCMCStrategy, Strategy)
    assert _fields(DefaultStrategy) == DEFAULT_FIELDS + [("reorder", False)]
    assert _fields(MCMCStrategy) == MCMC_FIELDS + [("reorder", False)]
    for f, (_, v) in zip(dataclasses.fields(DefaultStrategy), DEFAULT_FIELDS):
        assert type(f.default) is type(v), f.name
    for f, (_, v) in zip(dataclasses.fields(MCMCStrategy), MCMC_FIELDS):
        assert type(f.default) is type(v), f.name
    for name in ("duplicate", "split", "remove", "reset_opa", "relocate", "sample_add", "inject_noise_to_position",
                 "_update_param_with_optimizer", "_multinomial_sample"):
        assert callable(getattr(ops, name)), name
    DefaultStrategy(key_for_gradient="gradient_2dgs")  # accepted as a field
    from gscodec_studio_amd.relocation import compute_relocation  # noqa: F401


def test_initialize_state():
    st = MCMCStrategy().initialize_state()
    binoms = st["binoms"]
    assert set(st) == {"binoms"} and binoms.shape == (51, 51) and binoms.dtype == torch.float32
    want = torch.tensor([[float(math.comb(n, k)) if k <= n else 0.0 for k in range(51)] for n in range(51)], dtype=torch.float64)
    assert torch.equal(binoms, want.to(torch.float32))
    st = DefaultStrategy().initialize_state(scene_scale=2.5)
    assert st == {"grad2d": None, "count": None, "scene_scale": 2.5}
    st = DefaultStrategy(refine_scale2d_stop_iter=100).initialize_state()
    assert st == {"grad2d": None, "count": None, "scene_scale": 1.0, "radii": None}


def _trainer(n=6, skip=None, frozen=()):
    shapes = {"means": (n, 3), "scales": (n, 3), "quats": (n, 4), "opacities": (n,)}
    params = {k: torch.nn.Parameter(torch.zeros(s), requires_grad=k not in frozen) for k, s in shapes.items() if k != skip}
    optimizers = {k: torch.optim.Adam([p], lr=1e-3) for k, p in params.items() if p.requires_grad}
    return params, optimizers


@pytest.mark.parametrize("cls", [DefaultStrategy, MCMCStrategy])
def test_check_sanity(cls):
    strategy = cls()
    params, optimizers = _trainer()
    strategy.check_sanity(params, optimizers)
    params, optimizers = _trainer(frozen=("quats",))  # a frozen parameter needs no optimizer
    strategy.check_sanity(params, optimizers)
    for missing in ("means", "scales", "quats", "opacities"):
        params, optimizers = _trainer(skip=missing)
        with pytest.raises(AssertionError, match=f"{missing} is required"):
            strategy.check_sanity(params, optimizers)
    params, optimizers = _trainer()
    del optimizers["scales"]  # trainable, no optimizer
    with pytest.raises(AssertionError, match="same keys"):
        strategy.check_sanity(params, optimizers)
    params, optimizers = _trainer()
    optimizers["means"].add_param_group({"params": [torch.nn.Parameter(torch.zeros(2))]})
    with pytest.raises(AssertionError, match="exactly one param_group"):
        strategy.check_sanity(params, optimizers)


# ------------------------------------------------------------------------------------------------------------------------------
# the schedule: which operation fires at which step
# ------------------------------------------------------------------------------------------------------------------------------
DEFAULT_SETTINGS = [
    dict(),
    dict(refine_start_iter=3, refine_every=4, reset_every=20, refine_stop_iter=50),
    dict(refine_start_iter=0, refine_every=5, reset_every=15, pause_refine_after_reset=6, refine_stop_iter=61),
    dict(refine_start_iter=10, refine_every=3, reset_every=7, pause_refine_after_reset=2, refine_stop_iter=40),
]


@pytest.mark.parametrize("kw", DEFAULT_SETTINGS)
def test_default_schedule(monkeypatch, kw):
    strategy = DefaultStrategy(**kw)
    last = 70 if kw else 3300
    events = []
    step_now = [0]

    def stats(grad, radii, gaussian_ids, width, height, n_cameras, grad2d, count, radii_state=None):
        events.append((step_now[0], "stats"))
        grad2d.fill_(1.0)  # every gaussian above grow_grad2d
        count.fill_(1.0)

    monkeypatch.setattr(default_mod, "densify_stats", stats)
    monkeypatch.setattr(default_mod, "duplicate", lambda **k: events.append((step_now[0], "duplicate")))
    monkeypatch.setattr(default_mod, "split", lambda **k: events.append((step_now[0], "split")))
    monkeypatch.setattr(default_mod, "remove", lambda **k: events.append((step_now[0], "remove")))
    monkeypatch.setattr(default_mod, "reset_opa", lambda **k: events.append((step_now[0], "reset", k["value"])))
    monkeypatch.setattr(torch.cuda, "empty_cache", lambda: None)

    n = 4
    params = {"means": torch.zeros(n, 3), "quats": torch.ones(n, 4),
              "scales": torch.log(torch.tensor([[0.001] * 3, [0.001] * 3, [0.05] * 3, [0.5] * 3])),  # two small, one large, one huge
              "opacities": torch.tensor([3.0, -9.0, 3.0, 3.0])}  # the second below prune_opa
    info = {"width": 8, "height": 8, "n_cameras": 1, "radii": torch.ones(1, n, dtype=torch.int32), "gaussian_ids": None,
            "means2d": torch.zeros(1, n, 2, requires_grad=True)}
    info["means2d"].grad = torch.zeros(1, n, 2)
    state = strategy.initialize_state()
    for step in range(last):
        step_now[0] = step
        strategy.step_post_backward(params, {}, state, step, info)

    # the reference's conditions (default.py:162-201), written out
    want = []
    for step in range(last):
        if step >= strategy.refine_stop_iter:
            continue
        want.append((step, "stats"))
        if (step > strategy.refine_start_iter and step % strategy.refine_every == 0
                and step % strategy.reset_every >= strategy.pause_refine_after_reset):
            want += [(step, "duplicate"), (step, "split"), (step, "remove")]
        if step % strategy.reset_every == 0:
            want.append((step, "reset", strategy.prune_opa * 2.0))
    assert events == want
    assert any(e[1] == "split" for e in events) and any(e[1] == "reset" for e in events)


MCMC_SETTINGS = [
    dict(),
    dict(refine_start_iter=3, refine_every=4, refine_stop_iter=30, cap_max=130),
    dict(refine_start_iter=0, refine_every=7, refine_stop_iter=50, cap_max=100),
]


@pytest.mark.parametrize("kw", MCMC_SETTINGS)
def test_mcmc_schedule(monkeypatch, kw):
    strategy = MCMCStrategy(**kw)
    last = 60 if kw else 1300
    events = []
    step_now = [0]
    params = {"means": torch.zeros(100, 3), "opacities": torch.full((100,), 2.0)}
    params["opacities"][:3] = -9.0  # three dead gaussians

    def add(**k):
        events.append((step_now[0], "add", k["n"]))
        params["means"] = torch.zeros(len(params["means"]) + k["n"], 3)
        params["opacities"] = torch.cat([params["opacities"], torch.full((k["n"],), 2.0)])

    monkeypatch.setattr(mcmc_mod, "relocate", lambda **k: events.append((step_now[0], "relocate", int(k["mask"].sum()))))
    monkeypatch.setattr(mcmc_mod, "sample_add", add)
    monkeypatch.setattr(mcmc_mod, "inject_noise_to_position", lambda **k: events.append((step_now[0], "noise", k["scaler"])))
    monkeypatch.setattr(torch.cuda, "empty_cache", lambda: None)
    state = strategy.initialize_state()
    lr = 1.6e-4
    for step in range(last):
        step_now[0] = step
        strategy.step_post_backward(params, {}, state, step, {}, lr=lr)

    want, n = [], 100
    for step in range(last):
        if step < strategy.refine_stop_iter and step > strategy.refine_start_iter and step % strategy.refine_every == 0:
            want.append((step, "relocate", 3))
            n_new = max(0, min(strategy.cap_max, int(1.05 * n)) - n)
            if n_new > 0:
                want.append((step, "add", n_new))
            n += n_new
        want.append((step, "noise", lr * strategy.noise_lr))
    assert events == want
    assert len(params["means"]) == n <= strategy.cap_max
    assert any(e[1] == "add" for e in events) == (strategy.cap_max > 100)  # (cap_max = 100: full from the start, never adds)


# ------------------------------------------------------------------------------------------------------------------------------
# the native entry points refuse bad arguments before any launch; CPU tensors are refused, not emulated
# ------------------------------------------------------------------------------------------------------------------------------
def test_native_argument_validation():
    protos = B.prototypes()
    for name in ("gs_relocation", "gs_inject_noise", "gs_densify_stats"):
        assert name in protos, name
    p = 4096  # a non-null, aligned stand-in for a device pointer: every call below must fail before it is used
    with pytest.raises(RuntimeError, match="n_max"):
        B.call("gs_relocation", 8, p, p, p, p, 0, p, p, None)
    with pytest.raises(RuntimeError, match="null"):
        B.call("gs_relocation", 8, p, p, None, p, 51, p, p, None)
    with pytest.raises(RuntimeError, match="C must be"):
        B.call("gs_densify_stats", 0, 8, 0, p, 2, p, None, 1.0, 1.0, 8.0, p, p, None, None)
    with pytest.raises(RuntimeError, match="grad2d"):
        B.call("gs_densify_stats", 1, 8, 0, p, 2, p, None, 1.0, 1.0, 8.0, None, p, None, None)
    with pytest.raises(RuntimeError, match="stride"):
        B.call("gs_densify_stats", 1, 8, 0, p, 1, p, None, 1.0, 1.0, 8.0, p, p, None, None)
    with pytest.raises(RuntimeError, match="null"):
        B.call("gs_inject_noise", 8, p, None, p, p, p, 1.0, None)
    # N == 0: success, nothing launched
    B.call("gs_relocation", 0, None, None, None, None, 51, None, None, None)
    B.call("gs_inject_noise", 0, None, None, None, None, None, 1.0, None)
    B.call("gs_densify_stats", 1, 0, 0, None, 2, None, None, 1.0, 1.0, 8.0, None, None, None, None)


def test_cpu_tensors_are_refused():
    from gscodec_studio_amd._c_adapter import _C
    from gscodec_studio_amd.relocation import compute_relocation

    n = 5
    params, optimizers = _trainer(n)
    binoms = MCMCStrategy().initialize_state()["binoms"]
    mask = torch.tensor([True, False, True, False, False])
    with pytest.raises(RuntimeError, match="no CPU"):
        compute_relocation(torch.rand(n), torch.rand(n, 3), torch.ones(n, dtype=torch.int64), binoms)
    with pytest.raises(RuntimeError, match="no CPU"):
        _C.compute_relocation(torch.rand(n), torch.rand(n, 3), torch.ones(n, dtype=torch.int32), binoms, 51)
    for call in (lambda: ops.duplicate(params, optimizers, {}, mask), lambda: ops.split(params, optimizers, {}, mask),
                 lambda: ops.remove(params, optimizers, {}, mask), lambda: ops.reset_opa(params, optimizers, {}, 0.01),
                 lambda: ops.relocate(params, optimizers, {}, mask, binoms), lambda: ops.sample_add(params, optimizers, {}, 2, binoms),
                 lambda: ops.inject_noise_to_position(params, optimizers, {}, 1.0)):
        with pytest.raises(RuntimeError, match="no CPU"):
            call()
    assert all(len(p) == n for p in params.values())  # nothing was changed
    info = {"width": 8, "height": 8, "n_cameras": 1, "radii": torch.ones(1, n, dtype=torch.int32), "gaussian_ids": None,
            "means2d": torch.zeros(1, n, 2, requires_grad=True)}
    info["means2d"].grad = torch.zeros(1, n, 2)
    strategy = DefaultStrategy()
    with pytest.raises(RuntimeError, match="no CPU"):
        strategy.step_post_backward(params, optimizers, strategy.initialize_state(), 1, info)
    with pytest.raises(RuntimeError, match="no CPU"):
        MCMCStrategy().step_post_backward(params, optimizers, MCMCStrategy().initialize_state(), 1, {}, lr=1e-4)


def test_c_adapter_has_compute_relocation():
    from gscodec_studio_amd import _c_adapter

    assert callable(_c_adapter._C.compute_relocation)
    doc = " ".join(_c_adapter.__doc__.split())
    assert "compute_relocation" in doc
    out_of_scope = doc[doc.index("Not provided"):doc.index("What the adapter cannot do")]
    assert "compute_relocation" not in out_of_scope and "Out of scope" not in doc
