"""CPU: bench.py's options and its --dump-outputs writer (seeded samples, float32 files, the 64 MiB bound)."""
import numpy as np
import torch

import bench


def test_plain_is_the_default_and_full_is_opt_in(monkeypatch):
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "out"


def test_dump_outputs_samples_large_arrays_the_same_way_every_time(tmp_path):
    g = torch.Generator().manual_seed(0)
    H, W, N = 1080, 1920, 100_000
    images = {"render_colors": torch.rand((1, H, W, 9), generator=g), "render_alphas": torch.rand((1, H, W, 1), generator=g)}
    per_splat = {"sh_grad": (torch.rand((N, 16, 3), generator=g, dtype=torch.float64), 0),
                 "radii": (torch.randint(0, 50, (1, N, 2), generator=g, dtype=torch.int32), 1)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), images, per_splat)
    out = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in ("render_colors", "render_alphas", "sh_grad", "radii")}
    for k, v in out.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / f"{k}.npy")), k
    assert out["render_alphas"].shape == (1, H, W, 1) and out["render_alphas"].dtype == np.float32  # small enough: whole
    assert out["render_colors"].shape == (bench.DUMP_IMAGE_BYTES // 36, 9)                             # too large: pixel sample
    assert out["sh_grad"].shape == (bench.DUMP_SPLAT_ROWS, 16, 3) and out["sh_grad"].dtype == np.float64
    assert out["radii"].shape == (1, bench.DUMP_SPLAT_ROWS, 2) and out["radii"].dtype == np.float32
    # the per-splat arrays share their rows: the sampled radii are the source's rows at the same indices
    rows = bench._seeded_rows(N, bench.DUMP_SPLAT_ROWS, 2)
    assert np.array_equal(out["radii"], per_splat["radii"][0][:, rows].numpy().astype(np.float32))
    assert np.array_equal(out["sh_grad"], per_splat["sh_grad"][0][rows].numpy())
    assert sum(v.nbytes for v in out.values()) <= bench.DUMP_LIMIT_BYTES


def test_splat_outputs_zero_what_the_projection_leaves_unwritten():
    radii = torch.tensor([[3, 0, 5]], dtype=torch.int32)
    meta = {"radii": radii, "means2d": torch.full((1, 3, 2), float("nan")), "depths": torch.tensor([[1.0, float("inf"), 2.0]]),
            "conics": torch.full((1, 3, 3), 7.0)}
    g = torch.zeros(3, 3, requires_grad=True)
    g.grad = torch.ones(3, 3)
    out = bench.splat_outputs({"means": g, "unused": torch.zeros(3, requires_grad=True)}, meta)
    assert sorted(out) == ["conics", "depths", "means2d", "means_grad", "radii"]
    assert out["means_grad"][1] == 0 and out["radii"][1] == 1
    assert torch.equal(out["depths"][0], torch.tensor([[1.0, 0.0, 2.0]]))
    assert torch.equal(out["conics"][0][0, :, 0], torch.tensor([7.0, 0.0, 7.0]))
    assert torch.isnan(out["means2d"][0][0, 0]).all() and (out["means2d"][0][0, 1] == 0).all()
