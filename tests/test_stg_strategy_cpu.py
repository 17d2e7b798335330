"""The spacetime densification strategies without a GPU: the public surface, the fields and defaults and the schedule against
tests/golden/stg_strategy.npz (the reference's own STG_Strategy.py / modified_stg.py run on the CPU), the sanity check, the
``temp_vis_mask`` rules, the argument validation of the two native entry points and the refusal of CPU tensors."""
import dataclasses
import json

import numpy as np
import pytest
import torch

from util import golden

from gscodec_studio_amd import _backend as B
from gscodec_studio_amd.strategy import Modified_STG_Strategy, STG_Strategy, Strategy, ops
from gscodec_studio_amd.strategy import stg as stg_mod

CLASSES = {"stg": STG_Strategy, "mod": Modified_STG_Strategy}
REQUIRED = ("means", "scales", "quats", "opacities", "trbf_scale", "trbf_center", "motion", "omega")
KEYS = REQUIRED + ("colors", "features_dir", "features_time")


def test_names_import_and_fields_equal_the_reference():
    import gscodec_studio_amd.strategy as S

    assert S.STG_Strategy is STG_Strategy and S.Modified_STG_Strategy is Modified_STG_Strategy
    fx = golden("stg_strategy.npz")
    for tag, cls in CLASSES.items():
        assert issubclass(cls, Strategy)
        want = [tuple(f) for f in json.loads(str(fx[f"fields_{tag}"]))]
        got = [(f.name, f.default) for f in dataclasses.fields(cls)]
        assert got == want + [("reorder", False)], tag
        for (_, g), (_, w) in zip(got, want):
            assert type(g) is type(w)
    assert STG_Strategy().refine_stop_iter == 9000
    assert "temp_vis_mask" in {f.name for f in dataclasses.fields(Modified_STG_Strategy)}
    assert "temp_vis_mask" not in {f.name for f in dataclasses.fields(STG_Strategy)}
    for cls in CLASSES.values():  # nothing on the instance before a mask was built, as in the reference
        assert not hasattr(cls(), "omegamask") and not hasattr(cls(), "rotationmask")
        for name in ("_update_state", "_grow_gs", "_prune_gs", "_zero_omegabymotion", "removeminmax"):
            assert callable(getattr(cls, name)), name
    assert callable(ops.stg_omega_mask) and callable(ops.stg_freeze_grads)


@pytest.mark.parametrize("cls", list(CLASSES.values()))
def test_initialize_state(cls):
    assert cls().initialize_state(scene_scale=2.5) == {"grad2d": None, "count": None, "scene_scale": 2.5}
    assert cls(refine_scale2d_stop_iter=100).initialize_state() == {"grad2d": None, "count": None, "scene_scale": 1.0, "radii": None}


def _trainer(n=6, skip=None):
    shapes = {"means": (n, 3), "scales": (n, 3), "quats": (n, 4), "opacities": (n,), "trbf_scale": (n, 1), "trbf_center": (n, 1),
              "motion": (n, 9), "omega": (n, 4)}
    params = {k: torch.nn.Parameter(torch.zeros(s)) for k, s in shapes.items() if k != skip}
    return params, {k: torch.optim.Adam([p], lr=1e-3) for k, p in params.items()}


@pytest.mark.parametrize("cls", list(CLASSES.values()))
def test_check_sanity_needs_the_eight_keys(cls):
    strategy = cls()
    strategy.check_sanity(*_trainer())
    for missing in REQUIRED:
        with pytest.raises(AssertionError, match=f"{missing} is required"):
            strategy.check_sanity(*_trainer(skip=missing))
    params, optimizers = _trainer()
    del optimizers["omega"]
    with pytest.raises(AssertionError, match="same keys"):
        strategy.check_sanity(params, optimizers)


# ------------------------------------------------------------------------------------------------------------------------------
# the schedule: which operation fires at which step, and what step_post_backward returns
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(CLASSES))
def test_schedule_trace_equals_the_reference(monkeypatch, tag):
    fx = golden("stg_strategy.npz")
    trace = json.loads(str(fx[f"trace_{tag}"]))
    assert len(trace) >= 10
    cls = CLASSES[tag]
    strategy = cls()
    N = fx["means"].shape[0]
    params = {k: torch.nn.Parameter(torch.tensor(fx[k])) for k in KEYS}
    optimizers = {k: torch.optim.Adam([p], lr=1e-3) for k, p in params.items()}
    state = {"scene_scale": float(fx["scene_scale"])}
    calls = []
    monkeypatch.setattr(stg_mod, "duplicate", lambda **k: calls.append("duplicate"))
    monkeypatch.setattr(stg_mod, "split", lambda **k: calls.append("split"))
    monkeypatch.setattr(stg_mod, "remove", lambda **k: calls.append("remove"))
    monkeypatch.setattr(stg_mod, "reset_opa", lambda **k: calls.append("reset_opa"))
    monkeypatch.setattr(stg_mod, "reorder_after_refine", lambda *a, **k: calls.append("reorder"))  # (reorder=False: never)

    def omega_mask(motion, scales, opacities, omega, *a, **k):
        calls.append("omega_mask")
        return torch.tensor(fx["omega_mask"]), torch.tensor(fx["omega_new"])

    def freeze(mask, omega_grad, quats_grad):
        assert mask.shape == (N, 1) and mask.dtype == torch.bool and omega_grad is params["omega"].grad
        calls.append("freeze")

    monkeypatch.setattr(stg_mod, "stg_omega_mask", omega_mask)
    monkeypatch.setattr(stg_mod, "stg_freeze_grads", freeze)
    monkeypatch.setattr(cls, "_update_state", lambda self, params, state, info, packed=False: calls.append("update_state"))
    monkeypatch.setattr(torch.cuda, "empty_cache", lambda: None)
    maxb, minb = [torch.tensor(v) for v in fx["maxbounds"]], [torch.tensor(v) for v in fx["minbounds"]]
    for row in trace:
        del calls[:]
        state["grad2d"], state["count"] = torch.tensor(fx["state_grad2d"]), torch.tensor(fx["state_count"])
        for k in ("omega", "quats"):
            params[k].grad = torch.ones(N, 4)
        ret = strategy.step_post_backward(params, optimizers, state, row["step"], {}, row["flag"], row["desicnt"], maxb, minb)
        assert calls == row["calls"], (row, calls)
        assert ret == row["returns"] and isinstance(ret, bool) == row["returns_bool"], (row, ret)
        if "duplicate" in row["calls"] and tag == "stg":  # the grow branch zeroes the statistics
            assert not state["grad2d"].any() and not state["count"].any()
    everything = {c for row in trace for c in row["calls"]}
    if tag == "stg":
        assert everything == {"update_state", "duplicate", "split", "remove", "reset_opa", "omega_mask", "freeze"}
        assert strategy.omegamask.shape == (N, 1) and torch.equal(strategy.rotationmask, ~strategy.omegamask)
        assert optimizers["omega"].param_groups[0]["params"][0] is params["omega"]  # the mask build replaced the parameter
        assert np.array_equal(params["omega"].detach().numpy(), fx["omega_new"])
    else:
        assert everything == {"update_state", "duplicate", "split", "remove", "reset_opa"}
        assert not hasattr(strategy, "omegamask")
        assert any(row["returns"] is True for row in trace)


def test_freeze_before_a_mask_exists_or_without_gradients_fails_as_in_the_reference():
    params, optimizers = _trainer()
    strategy = STG_Strategy()
    with pytest.raises(AttributeError, match="omegamask"):
        strategy.step_post_backward(params, optimizers, strategy.initialize_state(), 9000, {}, 0, 0, None, None)
    strategy.omegamask = torch.ones(6, 1, dtype=torch.bool)
    with pytest.raises(TypeError):  # omega.grad is None
        strategy.step_post_backward(params, optimizers, strategy.initialize_state(), 9000, {}, 0, 0, None, None)


# ------------------------------------------------------------------------------------------------------------------------------
# temp_vis_mask
# ------------------------------------------------------------------------------------------------------------------------------
def test_temp_vis_mask_rules():
    n = 6
    params, optimizers = _trainer(n)
    full = torch.zeros(1, n, 2, requires_grad=True) * 1.0  # (a non-leaf, as a renderer returns it)
    strategy = Modified_STG_Strategy(temp_vis_mask=True)
    with pytest.raises(AssertionError, match="2D means"):
        strategy.step_pre_backward(params, optimizers, {}, 1, {})
    with pytest.raises(AssertionError, match="temporal visible mask"):
        strategy.step_pre_backward(params, optimizers, {}, 1, {"means2d": full})
    info = {"means2d": full, "t_vis_mask": torch.ones(n, dtype=torch.bool)}
    strategy.step_pre_backward(params, optimizers, {}, 1, info)
    assert info["means2d"] is full and full.retains_grad  # kept, and its gradient will be there
    compact = torch.zeros(1, n - 2, 2, requires_grad=True) * 1.0
    with pytest.raises(ValueError, match="full-size"):
        strategy.step_pre_backward(params, optimizers, {}, 1, {"means2d": compact, "t_vis_mask": torch.ones(n, dtype=torch.bool)})
    # without the option neither the mask nor the row count is looked at
    info = {"means2d": torch.zeros(1, n - 2, 2, requires_grad=True) * 1.0}
    Modified_STG_Strategy().step_pre_backward(params, optimizers, {}, 1, info)
    assert info["means2d"].retains_grad
    info = {"means2d": torch.zeros(1, n, 2, requires_grad=True) * 1.0}
    STG_Strategy().step_pre_backward(params, optimizers, {}, 1, info)
    assert info["means2d"].retains_grad
    doc = " ".join(Modified_STG_Strategy.__doc__.split())
    assert "temp_vis_mask" in doc and "difference" in doc and "ValueError" in doc


# ------------------------------------------------------------------------------------------------------------------------------
# the native entry points refuse bad arguments before any launch; CPU tensors are refused, not emulated
# ------------------------------------------------------------------------------------------------------------------------------
def test_native_argument_validation():
    protos = B.prototypes()
    assert len(protos["gs_stg_omega_mask"][1]) == 13 and len(protos["gs_stg_freeze_grads"][1]) == 5
    p, q = 4096, 8192  # non-null, aligned stand-ins for device pointers: every call below must fail before they are used
    with pytest.raises(RuntimeError, match="motion_row_stride"):
        B.call("gs_stg_omega_mask", 8, p, 2, p, p, p, 0.3, 0.2, 0.6, 0.7, p, q, None)
    with pytest.raises(RuntimeError, match="null input"):
        B.call("gs_stg_omega_mask", 8, p, 9, None, p, p, 0.3, 0.2, 0.6, 0.7, p, q, None)
    with pytest.raises(RuntimeError, match="null mask"):
        B.call("gs_stg_omega_mask", 8, p, 9, p, p, p, 0.3, 0.2, 0.6, 0.7, None, q, None)
    with pytest.raises(RuntimeError, match="4-byte aligned"):
        B.call("gs_stg_omega_mask", 8, p + 2, 9, p, p, p, 0.3, 0.2, 0.6, 0.7, p, q, None)
    with pytest.raises(RuntimeError, match="null mask"):
        B.call("gs_stg_freeze_grads", 8, None, p, q, None)
    with pytest.raises(RuntimeError, match="null omega_grad"):
        B.call("gs_stg_freeze_grads", 8, p, None, q, None)
    with pytest.raises(RuntimeError, match="different arrays"):
        B.call("gs_stg_freeze_grads", 8, p, q, q, None)
    # N == 0: success, nothing launched
    B.call("gs_stg_omega_mask", 0, None, 9, None, None, None, 0.3, 0.2, 0.6, 0.7, None, None, None)
    B.call("gs_stg_freeze_grads", 0, None, None, None, None)


def test_cpu_tensors_are_refused():
    n = 5
    params, optimizers = _trainer(n)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.stg_omega_mask(params["motion"], params["scales"], params["opacities"], params["omega"])
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.stg_freeze_grads(torch.ones(n, 1, dtype=torch.bool), torch.zeros(n, 4), torch.zeros(n, 4))
    with pytest.raises(TypeError, match="omega.grad"):
        ops.stg_freeze_grads(torch.ones(n, 1, dtype=torch.bool), None, torch.zeros(n, 4))
    with pytest.raises(TypeError, match="quats.grad"):
        ops.stg_freeze_grads(torch.ones(n, 1, dtype=torch.bool), torch.zeros(n, 4), None)
    for cls in CLASSES.values():
        with pytest.raises(RuntimeError, match="no CPU"):
            cls()._zero_omegabymotion(params, optimizers)
    assert all(len(p) == n for p in params.values())
