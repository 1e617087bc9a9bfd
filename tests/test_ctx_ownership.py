"""Who reaches into which part of the context (hector_slam_amd/csrc/hsm_ctx.h: hsm_ctx), without a GPU.

hsm_ctx groups its state into member structs by the unit that owns it.  REACH is the written record of every unit whose text names
a member: the owner, and each cross-unit coupling with its reason.  The test holds it EQUAL to what a scan of the .hip files finds,
so a new reach into another unit's state fails here until it is written down on purpose.  The core (hector_mi355.hip) is exempt:
it creates, parses and frees everything."""
import os
import re

from hector_slam_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "hector_slam_amd", "csrc")
CORE = "hector_mi355.hip"

# what every unit may use (the layout is a setting, and the one every sampler launch reads)
SHARED = {"bufs", "device", "compute_units", "levels", "start", "mu", "stream", "d_scan", "d_batch", "cfg.layout"}

# member struct (the settings: cfg and its group) -> the units that name it.  First the owner(s), then who else and why.
REACH = {
    # ---- settings (settings.h): read-only outside the core
    "cfg.parity": {"match.hip"},  # (everyone else asks wants_exact)
    "cfg.match": {"match.hip"},
    "cfg.batch": {"match.hip", "match_teams.hip", "match_exact_cached.hip",
                  "probes.hip"},  # hsm_debug_batch_order reads the order it is to show
    "cfg.single": {"match.hip"},
    "cfg.upd": {"map_update.hip"},
    "cfg.forms": {"rays.hip", "window.hip", "map_copy.hip"},  # one field each
    # ---- state
    "order": {"map_update.hip", "map_copy.hip", "map_shift.hip"},  # the core's; the three map writers that refuse while a stream the
                                                                   # context matches on is captured walk `foreign` themselves
    "single": {"match.hip",
               "probes.hip"},  # the debug hooks write the matcher's state (coop mute, fallback count); the probes borrow d_small
    "batch": {"match.hip", "match_teams.hip", "match_exact_cached.hip",
              "probes.hip"},  # the debug hooks (schedule, speculation statistics)
    "last": {"match.hip", "match_teams.hip", "rays.hip", "window.hip"},  # the launch record: whoever launches writes it
    "retained": {"match.hip", "map_update.hip"},  # matchData hands its scan to updateByScan
    "upd": {"map_update.hip",
            "map_copy.hip", "map_shift.hip", "probes.hip",  # upd_boxes_outstanding / gate_outstanding: folded before the host reads a level
            "match.hip"},  # queued_update: a drained stream clears it, the overlapped scan upload asks it
    "ingest": {"ingest.hip",
               "match.hip", "map_update.hip"},  # the ingested scan is matched and integrated
    "occ": {"occupancy.hip",
            "map_update.hip", "map_shift.hip"},  # d_pub_boxes: device-side updates widen the publish boxes, a window move resets them
    "copy": {"map_copy.hip", "map_shift.hip"},  # (the shift borrows the staging patch)
    "d_cells": {"probes.hip"},
}


def _reaches(unit):
    """the members of the context that `unit` names through any hsm_ctx pointer it declares, comments left out"""
    text = open(os.path.join(CSRC, unit)).read()
    text = re.sub(r"//[^\n]*", "", text)
    pointers = set(re.findall(r"\bhsm_ctx\s*\*\s*(?:const\s+)?(\w+)", text))
    found = set()
    for p, name, sub in re.findall(r"\b(\w+)->(\w+)(?:\.(\w+))?", text):
        if p in pointers:
            found.add("cfg." + sub if name == "cfg" else name)
    return found


def test_every_access_outside_the_core_names_a_member_struct_or_a_shared_field():
    for unit in build.UNITS:
        if unit != CORE:
            assert _reaches(unit) <= SHARED | set(REACH), unit


def test_reach_table_is_what_the_units_do():
    found = {member: set() for member in REACH}
    for unit in build.UNITS:
        if unit != CORE:
            for member in _reaches(unit) - SHARED:
                found[member].add(unit)
    assert found == REACH


def test_context_header_declares_the_members_of_the_table():
    header = open(os.path.join(CSRC, "hsm_ctx.h")).read()
    ctx = header[header.index("struct hsm_ctx {"):]
    for member in REACH:
        if not member.startswith("cfg."):
            assert re.search(r"[} ]%s(\{&bufs\})?;" % member, ctx), member
    settings = open(os.path.join(CSRC, "settings.h")).read()
    for member in REACH:
        if member.startswith("cfg."):
            assert re.search(r"\b%s( = [^;]+)?;" % member[4:], settings), member


def test_settings_header_is_hip_free():
    for path in build._closure(os.path.join(CSRC, "settings.h"), []):
        text = open(path).read()
        assert "hip_runtime" not in text and "hsm_ctx.h" not in text and not re.search(r'#\s*include\s*[<"]hip/', text), path
    names = {os.path.basename(p) for p in build._closure(os.path.join(CSRC, "settings.h"), [])}
    assert names == {"settings.h", "match_plan.h", "capi.h"}
