"""CPU: the directory layer under the three file codecs (gscodec_studio_amd/compression/_container.py) on its own -- the two
attribute loops with stub callbacks, the ordering dispatch, the preparation step and the plane file names."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from gscodec_studio_amd.compression import _container as C
from gscodec_studio_amd.compression import log_transform, morton_order
from gscodec_studio_amd.compression.stg_compression import STG_ATTRIBUTE_CODECS


def test_directory_loops_with_stub_callbacks(tmp_path):
    """One attribute with a zero in its shape, one that goes to npz, one the stub codes and one it defers: the files, the key
    order on both sides, the zeros and the npz attribute bit for bit."""
    g = torch.Generator().manual_seed(0)
    splats = {"late": torch.randn(6, 2, generator=g), "none": torch.zeros(6, 0, 3, dtype=torch.int32),
              "other": torch.randn(6, 2, 2, generator=g, dtype=torch.float64), "mine": torch.randn(6, generator=g)}
    seen = []

    def encode(name, value, meta):
        seen.append((name, list(meta)))
        if name in ("mine", "late"):
            value.numpy().tofile(os.path.join(d, f"{name}.raw"))
            return {**C.meta_of(value), "tag": name}
        return None

    d = str(tmp_path / "new" / "dir")  # created by the layer
    C.write_directory(d, splats, encode)
    assert seen == [("late", []), ("other", ["late", "none"]), ("mine", ["late", "none", "other"])]  # never the empty one
    assert sorted(os.listdir(d)) == ["late.raw", "meta.json", "mine.raw", "other.npz"]
    with open(os.path.join(d, "meta.json")) as f:
        meta = json.load(f)
    assert list(meta) == list(splats)
    assert meta["none"] == {"shape": [6, 0, 3], "dtype": "int32"} and meta["other"] == {"shape": [6, 2, 2], "dtype": "float64"}
    assert meta["mine"] == {"shape": [6], "dtype": "float32", "tag": "mine"}
    assert list(np.load(os.path.join(d, "other.npz")).files) == ["arr"]

    deferred = {}

    def decode(name, m, so_far):
        assert name != "none" and list(so_far) == list(meta)[: list(meta).index(name)]
        if name == "late":
            deferred[name] = m
            return C.DEFERRED
        if name == "mine":
            return torch.from_numpy(np.fromfile(os.path.join(d, "mine.raw"), np.float32)).reshape(m["shape"])
        return None

    out = C.read_directory(d, decode, "cpu")
    assert list(out) == list(meta) and out["late"] is None and list(deferred) == ["late"]
    out["late"] = torch.from_numpy(np.fromfile(os.path.join(d, "late.raw"), np.float32)).reshape(deferred["late"]["shape"])
    assert list(out) == list(meta)  # filled in place: the position is the meta's
    assert out["none"].shape == (6, 0, 3) and out["none"].dtype == torch.int32
    for k in ("late", "other", "mine"):
        assert out[k].dtype == splats[k].dtype and torch.equal(out[k], splats[k]), k


def _splats(n, seed=1):
    g = torch.Generator().manual_seed(seed)
    return {"means": torch.randn(n, 3, generator=g) * 4, "quats": torch.randn(n, 4, generator=g),
            "opacities": torch.randn(n, generator=g), "id": torch.arange(n)}


def test_order_splats(monkeypatch):
    splats = _splats(49)
    same = C.order_splats(splats, False, False)
    assert list(same) == list(splats) and all(same[k] is splats[k] for k in splats)
    order = morton_order(splats["means"])
    assert not torch.equal(order, torch.arange(49))
    got = C.order_splats(splats, "morton", False)
    assert list(got) == list(splats) and all(torch.equal(got[k], splats[k][order]) for k in splats)
    monkeypatch.setitem(sys.modules, "plas", None)
    for use_sort in (True, "plas", 1):  # whatever else is true means PLAS
        with pytest.raises(ImportError, match="PLAS"):
            C.order_splats(splats, use_sort, False)


def test_prepare_splats(capsys):
    n = 7 * 7 + 5
    splats = _splats(n)
    splats["opacities"][[3, 20, 41]] = torch.tensor([-6.0, -7.0, -8.0])  # sigmoid < 0.005; everything else is above it
    assert int((torch.sigmoid(splats["opacities"]) < 0.005).sum()) == 3
    before = {k: v.clone() for k, v in splats.items()}
    by_opacity = torch.argsort(splats["opacities"], descending=True)

    kept, side = C.prepare_splats(splats, None, False, False)  # no filter: every splat up to the crop, the lowest five go
    assert side == 7 and list(kept) == list(splats) and torch.equal(kept["id"], by_opacity[:49])
    assert capsys.readouterr().out == ""
    assert torch.equal(kept["means"], log_transform(splats["means"][kept["id"]]))
    assert torch.equal(kept["quats"], torch.nn.functional.normalize(splats["quats"][kept["id"]], dim=-1))
    assert torch.equal(kept["opacities"], splats["opacities"][kept["id"]])

    kept, side = C.prepare_splats(splats, 0.005, False, True)  # the three below the threshold, then the lowest two of the rest
    assert side == 7 and torch.equal(kept["id"], by_opacity[:49]) and not set(kept["id"].tolist()) & {3, 20, 41}
    assert "Removed 2 Gaussians" in capsys.readouterr().out
    filtered = torch.sigmoid(splats["opacities"]) >= 0.005
    assert set(torch.arange(n)[filtered].tolist()) - set(kept["id"].tolist()) == set(by_opacity[49:51].tolist())

    # the spacetime codec's parameters: its own normaliser, and the crop announced without ``verbose``
    kept, _ = C.prepare_splats(splats, None, "morton", False, normalize_quats=lambda q: q * 2, always_warn=True)
    assert "Removed 5 Gaussians" in capsys.readouterr().out
    order = by_opacity[:49][morton_order(log_transform(splats["means"][by_opacity[:49]]))]
    assert torch.equal(kept["id"], order) and torch.equal(kept["quats"], splats["quats"][order] * 2)

    assert list(splats) == list(before) and all(torch.equal(splats[k], before[k]) for k in before)  # the caller's dict is untouched


def test_plane_files():
    assert C.plane_files("sh0") == ("sh0.png",) and C.plane_files("scales", "kbit") == ("scales.png",)
    assert C.plane_files("means", "16") == ("means_l.png", "means_u.png")
    assert C.plane_files("motion", "multi", 3) == ("motion_0.png", "motion_1.png", "motion_2.png")
    assert C.plane_files("motion", "multi", 4)[-1] == "motion_3.png"
    for name, (kind, bits, files) in STG_ATTRIBUTE_CODECS.items():
        assert C.plane_files(name, kind, 3) == tuple(files) and len(files) == {"16": 2, "multi": 3}.get(kind, 1), name
