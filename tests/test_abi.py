"""CPU: the C-ABI library loads and exports every symbol include/gsplat_hip.h declares, the
header-derived ctypes prototypes are sane, and the product fails loudly (no fallback) when the
library is missing or when it is handed CPU tensors.  No compute calls are made here."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from gscodec_studio_amd import _backend as B

    protos = B.parse_header()
    assert len(protos) >= 24
    lib = ctypes.CDLL(B.LIB_PATH)
    for name in protos:
        assert hasattr(lib, name), f"{name} declared in include/gsplat_hip.h but not exported"
    # and nothing with the gs_ prefix is exported without being declared
    out = subprocess.check_output(["nm", "-D", "--defined-only", B.LIB_PATH], text=True)
    exported = set(re.findall(r"\bT (gs_\w+)", out))
    assert exported == set(protos), exported ^ set(protos)


def test_abi_v6_version_and_error_string():
    """ABI 6: gs_step without the backward half (gs_step_bwd and the fields only it read are gone)."""
    from gscodec_studio_amd import _backend as B

    L = B.lib()
    assert L.gs_version() == B.header_abi_version() == 6
    assert L.gs_header_hash() == B.header_hash()  # the library was compiled against THIS header
    assert isinstance(L.gs_last_error(), bytes)
    assert B.query("gs_sort_temp_bytes", 1000) >= 1000 * 12
    assert B.query("gs_cumsum_scratch_bytes", 10_000) >= 8
    from gscodec_studio_amd import _wrapper as W

    plan, sb = W._raster_plan(8160, 4_000_000, 3)
    assert sb > 4_000_000 // 256 * 4 * 256 * 4  # checkpoint planes every 256 entries
    import struct

    magic, n_tiles, n_isects, channels, seg, solo = struct.unpack_from("<IIIIii", plan, 0)
    assert (n_tiles, n_isects, channels, seg, solo) == (8160, 4_000_000, 3, 256, 2048)
    prev = W.set_raster_tuning(raster_seg=100, raster_solo_min=0)  # rounded up to a multiple of 64
    try:
        plan2, sb2 = W._raster_plan(8160, 4_000_000, 3)
        assert struct.unpack_from("<ii", plan2, 16) == (128, 0) and sb2 > sb
    finally:
        W.set_raster_tuning(**prev)


def test_stale_header_or_library_is_refused(tmp_path):
    """A header that does not match the library (other version, or same version but different text) must fail the import,
    not be called through shifted argument lists."""
    from gscodec_studio_amd import _backend as B

    src = open(B.HEADER_PATH).read()
    for name, text, expect in (("ver.h", re.sub(r"#define GS_ABI_VERSION \d+", "#define GS_ABI_VERSION 2", src), "ABI version mismatch"),
                               ("txt.h", src.replace("gs_stream_t stream);", "gs_stream_t  stream);", 1), "different gsplat_hip.h")):
        h = tmp_path / name
        h.write_text(text)
        code = "import gscodec_studio_amd._backend as B; B.lib()"
        env = dict(os.environ, GSPLAT_HIP_HEADER=str(h), PYTHONPATH=ROOT)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
        assert r.returncode != 0 and expect in r.stderr, (name, r.stderr[-500:])


def test_argument_validation_happens_before_any_launch():
    """Status codes + messages for bad arguments (no GPU needed: the checks precede the launch)."""
    from gscodec_studio_amd import _backend as B

    with pytest.raises(RuntimeError, match="exactly one of covars"):
        B.call("gs_projection_fwd", 1, 1, 1, None, None, None, 1, 1, 10, 10, 0.3, 0.01, 1e10, 0.0, 0, 1, 1, 1, 1, None, None)
    with pytest.raises(RuntimeError, match="degree must be <= 4"):
        B.call("gs_sh_fwd", 1, 1, 36, 5, 1, 1, 0, None, 1, None)
    with pytest.raises(RuntimeError, match="unsupported number of colour channels"):
        B.call("gs_rasterize_fwd", 1, 1, 0, 600, None, None, None, None, None, None, None, 16, 16, 16, 1, 1, 1, None, 1, 1, 1, None, None, None, 0, None)
    with pytest.raises(RuntimeError, match="tile_size must be in"):
        B.call("gs_rasterize_fwd", 1, 1, 0, 3, None, None, None, None, None, None, None, 16, 16, 32, 1, 1, 1, None, 1, 1, 1, None, None, None, 0, None)
    with pytest.raises(RuntimeError, match="plan and scratch go together"):
        B.call("gs_rasterize_fwd", 1, 1, 0, 3, None, None, None, None, None, None, None, 16, 16, 16, 1, 1, 1, None, 1, 1, 1, None, 1, None, 0, None)
    with pytest.raises(RuntimeError, match="temp too small"):
        B.call("gs_sort_pairs_u64_i32", 10, 1, 1, 1, 1, 0, 40, None, 0, None)


def test_missing_library_fails_loudly():
    code = "import gscodec_studio_amd._backend as B; B.lib()"
    env = dict(os.environ, GSPLAT_HIP_LIB="/nonexistent/libgsplat_hip.so", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode != 0 and "native library not found" in r.stderr and "no CPU fallback" in r.stderr.replace("There is no", "no")


def test_cpu_tensors_are_rejected_not_emulated():
    import gscodec_studio_amd as g
    from gscodec_studio_amd.compression_simulation import fake_quantize_ste

    N = 8
    means, quats, scales = torch.randn(N, 3), torch.randn(N, 4), torch.rand(N, 3)
    viewmats, Ks = torch.eye(4)[None], torch.eye(3)[None]
    with pytest.raises(RuntimeError, match="no CPU"):
        g.fully_fused_projection(means, None, quats, scales, viewmats, Ks, 32, 32)
    with pytest.raises(RuntimeError, match="no CPU"):
        g.spherical_harmonics(0, torch.randn(N, 3), torch.randn(N, 1, 3))
    with pytest.raises(RuntimeError, match="no CPU"):
        g.rasterization(means, quats, scales, torch.rand(N), torch.rand(N, 3), viewmats, Ks, 32, 32)
    with pytest.raises(RuntimeError, match="no CPU"):
        fake_quantize_ste(torch.randn(10), -1, 1, 8, "round")


def test_host_struct_mirrors_match_the_library_layout(tmp_path):
    """The host structs that cross the boundary by pointer (gs_step, gs_quant_desc, gs_adam_desc) are ctypes classes derived from
    the header: the library reports its own sizeof / offsetof (gs_step_layout, gs_quant_desc_layout, gs_adam_desc_layout) and the
    classes must agree; a header that drifted from the library is refused before a descriptor is ever handed over.  Names and order
    come from the header too, so two same-typed neighbours cannot be swapped behind the guard's back."""
    from gscodec_studio_amd import _backend as B
    from gscodec_studio_amd import _step, _wrapper
    from gscodec_studio_amd.compression_simulation import ops

    B.check_layouts()  # gs_step, gs_quant_desc and gs_adam_desc, each against its own entry point
    assert set(B._LAYOUT_GUARDS) == {"gs_step", "gs_quant_desc", "gs_adam_desc"}
    # what lib() guarded (the default header's classes) are the very objects the modules build their descriptors from
    guarded = B._header().structs
    assert B._header() is B._header(B.HEADER_PATH)
    assert _step._Step is guarded["gs_step"] and ops._QuantDesc is guarded["gs_quant_desc"] and _wrapper._AdamDesc is guarded["gs_adam_desc"]
    assert _wrapper._RasterPlan is guarded["gs_raster_plan"] is dict(_step._Step._fields_)["plan"]
    for name, (entry, guarded) in B._LAYOUT_GUARDS.items():  # (gs_step_layout(None, 0) == 1 + len(its guarded field list), and so on)
        assert int(B.query(entry, None, 0)) == 1 + len(guarded), name

    src = open(B.HEADER_PATH).read()
    # a field too many in the middle of gs_step: everything behind it moves
    drift = tmp_path / "drift.h"
    anchor = "    uint32_t sh_K, sh_degree;\n"
    assert src.count(anchor) == 1
    drift.write_text(src.replace(anchor, anchor + "    uint64_t extra;\n"))
    assert "extra" in [f[0] for f in B.struct("gs_step", str(drift))._fields_]
    with pytest.raises(ImportError, match="struct layout"):
        B.check_layouts(str(drift))

    # two same-typed neighbours swapped (what a hand-written mirror could get wrong unnoticed): the class follows the header
    swap = tmp_path / "swap.h"
    pointers = "const float *means, *covars, *quats"
    assert src.count(pointers) == 1
    swap.write_text(src.replace(pointers, "const float *covars, *means, *quats").replace(
        "uint32_t tile_size, tile_width, tile_height;", "uint32_t tile_size, tile_height, tile_width;"))
    real = [f[0] for f in B.struct("gs_step")._fields_]
    swapped = [f[0] for f in B.struct("gs_step", str(swap))._fields_]
    assert real != swapped and sorted(real) == sorted(swapped)
    assert real.index("means") + 1 == real.index("covars") and swapped.index("covars") + 1 == swapped.index("means")
    assert real.index("tile_width") + 1 == real.index("tile_height") and swapped.index("tile_height") + 1 == swapped.index("tile_width")


def test_product_never_imports_the_oracle():
    """The oracle is test infrastructure: nothing under gscodec_studio_amd/ may reference it."""
    pkg = os.path.join(ROOT, "gscodec_studio_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M), os.path.join(dirpath, f)
                assert "gs_oracle" not in src, os.path.join(dirpath, f)
