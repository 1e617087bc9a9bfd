"""The C-ABI shared library builds for gfx950, loads, and exports every symbol that
include/hector_mi355/capi.h declares.  No compute calls (runs without a GPU)."""
import os
import re

import pytest

from support import compile_c99, header_code

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    return sorted(set(re.findall(r"\b(hsm_[a-z0-9_]+)\s*\(", header_code())))


def test_header_and_binding_agree():
    from hector_slam_amd import capi
    decl = declared_symbols()
    assert len(decl) >= 25
    assert sorted(capi.SIGNATURES) == decl


def test_library_builds_loads_and_exports_all_symbols():
    from hector_slam_amd import build, capi
    path = build.build_native()
    assert os.path.exists(path)
    lib = capi.load_library()
    for name in declared_symbols():
        assert hasattr(lib, name), name
    assert b"gfx950" in lib.hsm_version()
    # the code object really targets gfx950
    blob = open(path, "rb").read()
    assert b"gfx950" in blob


def test_no_cpu_fallback_without_device():
    import torch
    from hector_slam_amd import capi
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the failure path is for GPU-less hosts")
    with pytest.raises(capi.HsmError):
        capi.MapRepMultiMap(0.05, 256, 256, 3)


def test_product_never_references_the_oracle():
    """oracle/ is test infrastructure: nothing under hector_slam_amd/ or include/ may mention it."""
    bad = []
    for base in ("hector_slam_amd", "include"):
        for dp, _, fns in os.walk(os.path.join(ROOT, base)):
            for fn in fns:
                if fn.endswith((".py", ".h", ".hip", ".cpp")):
                    txt = open(os.path.join(dp, fn), errors="ignore").read()
                    if re.search(r"\bimport\s+oracle|from\s+oracle|oracle/|libhector_oracle|libhector_ref|pyoracle", txt):
                        bad.append(os.path.join(dp, fn))
    assert not bad, bad


def test_header_is_plain_c99(tmp_path):
    """the boundary is a C ABI: the header must compile as C (what cgo / JNI / ctypes-style bindings consume)"""
    compile_c99(tmp_path,
                'int main(void) { hsm_ctx* h = 0; hsm_opts o = {-1, HSM_LAYOUT_AUTO, 0}; (void)o;\n'
                '  return hsm_create(0.05f, 64, 64, 1u, 0.5f, 0.5f, &o, &h) == HSM_OK ? 0 : 1; }\n')


def test_rccl_is_loaded_on_demand_not_linked():
    """north_star's "RCCL gather of the 3-DoF poses" lives in the C++ group (hsm_group_match_batch_device): librccl is
    dlopen'ed by the group's first device gather, so the single-GPU library keeps its dependency set (HIP / HSA / libc) --
    and the RCCL this image ships exports every entry point the group binds"""
    import ctypes
    import subprocess
    from hector_slam_amd import build
    path = build.build_native()
    needed = subprocess.run(["readelf", "-d", path], capture_output=True, text=True, check=True).stdout
    assert "rccl" not in needed.lower() and "nccl" not in needed.lower(), needed
    blob = open(path, "rb").read()
    for sym in (b"ncclCommInitAll", b"ncclAllGather", b"ncclGroupStart", b"ncclGroupEnd", b"ncclSend", b"ncclRecv",
                b"ncclCommDestroy", b"librccl.so.1"):
        assert sym in blob, sym  # the names the group resolves with dlsym
    try:
        rccl = ctypes.CDLL("librccl.so.1")
    except OSError as e:  # pragma: no cover - the image ships RCCL
        pytest.skip(f"librccl.so.1 not loadable here: {e}")
    for sym in ("ncclCommInitAll", "ncclAllGather", "ncclGroupStart", "ncclGroupEnd", "ncclSend", "ncclRecv", "ncclCommDestroy",
                "ncclGetErrorString", "ncclGetVersion"):
        assert hasattr(rccl, sym), sym
