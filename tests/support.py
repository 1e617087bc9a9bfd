"""Fixtures and helpers that the tests share.  A test file imports what it needs from here (`from support import capi, same`)
and does not copy it; pytest finds a fixture that is imported into a test module's namespace.  What is specific to one feature
(its geometries, its device driver, its tolerant comparisons) stays in that feature's files."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import bits, oracle_kinds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hector_slam_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")


# ---- fixtures ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def capi():
    import torch
    assert torch.cuda.is_available(), "gpu-marked tests need a HIP device"
    from hector_slam_amd import capi as m
    m.load_library()  # raises if the native library is missing: no silent fallback
    return m


@pytest.fixture(scope="module", params=oracle_kinds())
def kind(request):
    """which CPU checker: "ho" = restatement, "hr" = the reference's own headers"""
    return request.param


# ---- arrays ------------------------------------------------------------------------------------------------------------
def same(a, b):
    """bit for bit as float32 (so 0.0 is not -0.0, and a NaN equals only the same NaN)"""
    return np.array_equal(bits(a), bits(b))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def stream_ptr():
    """the current torch stream as the hipStream_t value the entries take"""
    import torch
    return torch.cuda.current_stream().cuda_stream


_hip = None


def hip_runtime():
    """the HIP runtime this process has loaded (the one the library and torch are bound to), as a ctypes handle"""
    global _hip
    if _hip is None:
        import ctypes
        paths = {line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line}
        assert len(paths) == 1, f"expected one loaded libamdhip64, found {sorted(paths)}"
        _hip = ctypes.CDLL(paths.pop())
        _hip.hipMemcpy.restype = ctypes.c_int
        _hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return _hip


def device_to_host(ptr, shape, dtype=np.float32):
    """what a raw device pointer holds, as a host array of `shape`: a blocking hipMemcpy, device to host"""
    assert ptr, "null device pointer"
    out = np.empty(shape, dtype)
    rc = hip_runtime().hipMemcpy(out.ctypes.data, int(ptr), out.nbytes, 2)  # hipMemcpyDeviceToHost
    assert rc == 0, f"hipMemcpy failed ({rc})"
    return out


def pack(scans):
    """a scan log as CSR: float32 points [n, 2] and int32 offsets [len(scans) + 1]; an empty log is a (0, 2) array"""
    offs = np.zeros(len(scans) + 1, np.int32)
    offs[1:] = np.cumsum([len(s) for s in scans])
    pts = np.concatenate([np.asarray(s, np.float32).reshape(-1, 2) for s in scans]) if offs[-1] else np.zeros((0, 2), np.float32)
    return np.ascontiguousarray(pts, np.float32), offs


# ---- device contexts and their checkers --------------------------------------------------------------------------------
def layout_of(capi, name):
    return capi.LAYOUT_QUAD if name == "quad" else capi.LAYOUT_PLANE


def new_context(capi, res, sx, sy, levels, start=(0.5, 0.5), layout="quad", factors=(0.4, 0.9), **kw):
    """a cleared context with the update factors set (factors=None leaves the library's own)"""
    g = capi.MapRepMultiMap(res, sx, sy, levels, startCoords=start, layout=layout_of(capi, layout), **kw)
    if factors is not None:
        g.setUpdateFactorFree(factors[0])
        g.setUpdateFactorOccupied(factors[1])
    return g


def single_update(capi, g, pose, pts, origo=(0.0, 0.0)):
    """hsm_retain_scan (what matchData leaves for the coarse levels) + hsm_update_by_scan, which returns when it is queued"""
    a = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    o = np.ascontiguousarray(origo, np.float32)
    capi._check(g._lib.hsm_retain_scan(g._h, a.ctypes.data, a.shape[0], o), "hsm_retain_scan")
    g.updateByScan(a, pose, o)


def new_refs(oracle_mod, res, sx, sy, levels, start=None, factors=(0.4, 0.9), kinds=None):
    """one checker per kind with the update factors set; `start` reaches Oracle only when the caller gives one"""
    refs = {}
    for kind in (kinds or oracle_kinds()):
        o = oracle_mod.Oracle(kind, res, sx, sy, levels, *(() if start is None else (start,)))
        o.set_update_factor_free(factors[0])
        o.set_update_factor_occupied(factors[1])
        refs[kind] = o
    return refs


def upload_planes(m, planes):
    """one (log-odds, update index) pair per level into a checker (pyoracle.Oracle) or a device context
    (capi.MapRepMultiMap): both have upload_level"""
    for lvl, (lo, ui) in enumerate(planes):
        m.upload_level(lvl, lo, ui)
    return m


# ---- the C header and the host-side check programs ---------------------------------------------------------------------
def header_text():
    return open(os.path.join(INCLUDE, "hector_mi355", "capi.h")).read()


def header_code():
    """the header without its block comments"""
    return re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)


def check_symbols(names, restype=r"int"):
    """each name is declared in capi.h with that return type, bound in capi.SIGNATURES with as many arguments as the
    declaration has, and exported by the built library"""
    from hector_slam_amd import build, capi
    code = header_code()
    build.build_native()
    lib = capi.load_library()
    for name in names:
        assert re.search(r"\b" + restype + r"\s+" + name + r"\s*\(", code), name
        assert name in capi.SIGNATURES, name
        assert hasattr(lib, name), name
        decl = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", code, re.S).group(1)
        assert len(capi.SIGNATURES[name][1]) == decl.count(",") + 1, (name, decl)


def compile_c99(tmp_path, body):
    """a translation unit that includes the header and holds `body` compiles as strict C99 without a warning"""
    src = tmp_path / "use.c"
    src.write_text('#include "hector_mi355/capi.h"\n' + body)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-c", str(src), "-I", INCLUDE,
                    "-o", str(tmp_path / "use.o")], check=True)


def build_check(dest_dir, source, *extra_flags):
    """compile tests/cpp/<source> against the library's headers into dest_dir; -> the executable's path"""
    exe = dest_dir / os.path.splitext(source)[0]
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, *extra_flags,
                    os.path.join(ROOT, "tests", "cpp", source), "-o", str(exe)], check=True)
    return exe
