"""The include graph of csrc/ without a GPU: a kernel header is reachable only from the unit that launches its kernels, the context
header sees types only, and the dependency table build.py derives from the #include lines is the compiler's own.
"""
import concurrent.futures
import os
import re
import subprocess

import pytest

from hector_slam_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "hector_slam_amd", "csrc")

# kernel-owning header -> the units that launch its kernels
OWNERS = {
    "gn_match_teams.h": {"match_teams.hip"},
    "gn_match_cached.h": {"match_teams.hip"},
    "gn_match_dense.h": {"match.hip"},
    "score_kernels.h": {"match.hip"},
    "probe_kernels.h": {"probes.hip"},
    "gn_match_exact.h": {"match_exact_cached.hip"},
    "gn_match_spec.h": {"match.hip"},
    "map_update.h": {"map_update.hip"},
    "map_update_scans.h": {"map_update.hip"},
    "update_types.h": {"map_update.hip"},
    "update_cell_rule.h": {"map_update.hip"},
    "update_gate.h": {"map_update.hip"},
}
# the kernel-free headers of the matcher: what the table says of them, as sets of units as well
ALL_BUT_EXCHANGE = set(build.UNITS) - {"pose_exchange.hip"}
SHARED = {
    "texel_cache.h": {"match_teams.hip", "match_exact_cached.hip"},
    "gn_step.h": {"match_teams.hip", "match_exact_cached.hip", "match.hip", "window.hip", "probes.hip"},
    "pose_score.h": {"match.hip", "window.hip", "probes.hip"},
    "match_types.h": ALL_BUT_EXCHANGE,
    "pose_exchange.h": set(build.UNITS),
}


def _names(paths):
    return {os.path.basename(p) for p in paths}


def _units_reaching(header):
    return {u for u, deps in build.UNITS.items() if header in _names(deps)}


def _closure_of(name):
    return build._closure(os.path.join(CSRC, name), [])


def test_fourteen_units_in_link_order():
    assert list(build.UNITS) == ["hector_mi355.hip", "match.hip", "map_update.hip", "ingest.hip", "occupancy.hip", "probes.hip",
                                 "rays.hip", "map_copy.hip", "map_shift.hip", "window.hip", "group.hip", "match_exact_cached.hip",
                                 "match_teams.hip", "pose_exchange.hip"]
    for unit, deps in build.UNITS.items():
        assert deps[0] == os.path.join(CSRC, unit) and all(os.path.isabs(d) and os.path.isfile(d) for d in deps), unit
        assert len(deps) == len(set(deps)), unit


@pytest.mark.parametrize("header", sorted(OWNERS))
def test_kernel_header_is_reached_by_its_launching_units_only(header):
    assert _units_reaching(header) == OWNERS[header]


@pytest.mark.parametrize("header", sorted(SHARED))
def test_shared_header_is_reached_by_its_users_only(header):
    assert _units_reaching(header) == SHARED[header]


def test_every_matcher_kernel_is_defined_in_one_header():
    where = {
        "gn_match_kernel": "gn_match_teams.h", "gn_match_cached_kernel": "gn_match_cached.h",
        "gn_match_exact_dense_kernel": "gn_match_dense.h", "gn_match_coop_kernel": "gn_match_dense.h",
        "score_batch_kernel": "score_kernels.h", "select_best_kernel": "score_kernels.h",
        "gn_eval_kernel": "probe_kernels.h", "gn_beam_terms_kernel": "probe_kernels.h",
        "likelihood_kernel": "probe_kernels.h", "pose_covariance_kernel": "probe_kernels.h",
    }
    for kernel, header in where.items():
        defined = [f for f in sorted(os.listdir(CSRC))
                   if re.search(r"__global__[^;{]*\b%s\s*\(" % kernel, open(os.path.join(CSRC, f)).read())]
        assert defined == [header], (kernel, defined)


def test_gn_match_h_is_gone():
    assert not os.path.exists(os.path.join(CSRC, "gn_match.h"))
    for f in sorted(os.listdir(CSRC)):
        assert not re.search(r'#\s*include\s*"gn_match\.h"', open(os.path.join(CSRC, f)).read()), f


def test_context_header_sees_types_only():
    closure = _closure_of("hsm_ctx.h")
    assert "match_types.h" in _names(closure)
    for path in closure:
        assert "__global__" not in open(path).read(), path
    # the matcher's types come with no device function at all
    assert "__device__" not in open(os.path.join(CSRC, "match_types.h")).read()
    assert not _names(closure) & {"beam_sample.h", "gn_step.h", "texel_cache.h"}


def test_cell_rule_header_is_plain_cpp():
    """both apply passes and the host's model test compile it: no HIP, nothing else of csrc/"""
    assert _names(_closure_of("update_cell_rule.h")) == {"update_cell_rule.h"}
    text = open(os.path.join(CSRC, "update_cell_rule.h")).read()
    assert "__global__" not in text and "hip_runtime" not in text


def test_exact_cached_unit_is_not_rebuilt_by_the_fast_kernels():
    deps = _names(build.UNITS["match_exact_cached.hip"])
    assert not deps & {"gn_match_cached.h", "gn_match_teams.h"}
    assert not _names(_closure_of("gn_match_exact.h")) & {"gn_match_cached.h", "gn_match_teams.h"}


def test_core_unit_launches_no_kernel():
    for path in _closure_of("hector_mi355.hip"):
        assert "__global__" not in open(path).read(), path
    core = open(os.path.join(CSRC, "hector_mi355.hip")).read()
    assert "hipLaunchKernelGGL" not in core and "hipLaunchCooperativeKernel" not in core


def test_matcher_front_door_does_not_see_the_kernels_it_dispatches_to():
    deps = _names(build.UNITS["match.hip"])
    assert not deps & {"map_update.h", "gn_match_exact.h", "gn_match_teams.h", "gn_match_cached.h"}


def _compiler_deps(hipcc, unit):
    cmd = [hipcc, "--cuda-host-only", "-MM", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(CSRC, unit)]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    words = out.replace("\\\n", " ").split(":", 1)[1].split()
    paths = {os.path.realpath(w) for w in words}
    return {p for p in paths if p.startswith(os.path.realpath(ROOT) + os.sep)}


@pytest.mark.skipif(build.hipcc_path() is None, reason="hipcc is absent")
def test_derived_table_is_the_compilers_dependency_list():
    hipcc = build.hipcc_path()
    assert "-std=c++17" in build.FLAGS
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        real = dict(zip(build.UNITS, ex.map(lambda u: _compiler_deps(hipcc, u), build.UNITS)))
    for unit, deps in build.UNITS.items():
        # no #include of csrc/ stands inside an #if, so the derived list is the compiler's, not a superset of it
        assert {os.path.realpath(d) for d in deps} == real[unit], unit
        assert "pose_exchange.h" in _names(real[unit]), unit  # (MatchParams holds an ExchangeFused: every object's layout)
