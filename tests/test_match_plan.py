"""The host runtime's choice of matcher form (hector_slam_amd/csrc/match_plan.h: plan_match) on the CPU.

tests/golden/match_forms.json holds, for a few hundred launch sites (tests/match_form_sites.py), what the library answered BEFORE
the plan existed -- kernel name, the five hsm_last_launch_config values, hsm_last_launch_parity -- recorded on a 256-CU MI355X by
tests/tools/record_match_forms.py.  tests/cpp/match_plan_check.cpp prints the plan of every site; the comparison is exact and no
site is skipped.  The same program checks by hand-written cases what the record cannot show (cached rows, the probe
instantiation, the carried exchange) and compares reads_scan_once with the literal restatement of the function it replaced."""
import json
import os
import subprocess

import pytest

import match_form_sites as mfs
from support import build_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "match_forms.json")
PARITY_WORD = {0: "fast", 1: "exact", 2: "relaxed"}
KERNEL_FAMILY = {  # the strings hsm_last_launch_kernel returns -> the families of the plan that may carry them
    "gn_match_kernel": {"team"}, "gn_match_kernel (exact order)": {"team_exact"}, "gn_match_cached_kernel": {"cached"},
    "gn_match_exact_cached_kernel": {"exact_cached"}, "gn_match_exact_cached_kernel (chain wavefront)": {"exact_cached_cw"},
    "gn_match_exact_cached_kernel + its chain-wavefront form for the last, part-filled generation": {"exact_cached"},
    "gn_match_exact_dense_kernel": {"exact_dense"}, "gn_match_spec_kernel": {"spec"}, "gn_match_spec1_kernel": {"spec1"},
    "gn_match_coop_kernel": {"coop"}}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return str(build_check(tmp_path_factory.mktemp("match_plan"), "match_plan_check.cpp"))


def flat(site, cu):
    """the MatchSite of a recorded site, as hsm_create and the two entry points fill it (match_plan_check.cpp: read_site)"""
    env = site["env"]
    sx, sy, _ = mfs.MAPS[site["map"]]
    batched = site["entry"] == "batch"
    f = [mfs.batch_of(site, cu) if batched else 1, site["n"], site["n"],
         int(site["parity"] in ("auto", "exact")), int(site["parity"] == "relaxed"), mfs.LAYOUT_CODE[site["layout"]],
         int(batched), 0, int(site["probe"]), 0, cu, sx * sy,
         int(env.get("HSM_WPS", 0)), 0 if int(env.get("HSM_BPL", -1)) == 0 else -1, int(int(env.get("HSM_TEXEL_CACHE", 1)) != 0),
         int(int(env.get("HSM_EXACT_CACHED", 1)) != 0), int(int(env.get("HSM_EXACT_CHAIN_WAVE", 1)) != 0),
         int(int(env.get("HSM_EXACT_SPLIT_TAIL", 1)) != 0), int(int(env.get("HSM_EXACT_DENSE", 1)) != 0),
         int(env.get("HSM_EXACT_DENSE_MIN", 4096)), int(int(env.get("HSM_EXACT_SPEC", 0)) != 0),
         int(int(env.get("HSM_EXACT_SPEC1", 0)) != 0), 8 if int(env.get("HSM_SPB_LARGE", 8)) == 8 else 4,
         int(env.get("HSM_COOP_MIN", 4096)), 0]
    return " ".join(str(v) for v in f)


def plans(check, golden):
    cu = golden["compute_units"]
    text = "\n".join(flat(s, cu) for s in golden["sites"]) + "\n"
    r = subprocess.run([check, "sites"], input=text, capture_output=True, text=True, check=True)
    out = []
    for line in r.stdout.splitlines():
        nums, name = line.split("|", 1)
        v = [int(x) for x in nums.split()]
        out.append({"family": mfs.FAMILIES[v[0]], "config": v[1:6], "parity": PARITY_WORD[v[6]], "kernel": name})
    return out


def test_the_table_is_the_recorded_list_and_covers_every_family_and_knob(golden):
    sites = golden["sites"]
    assert len(sites) >= 300 and golden["compute_units"] == 256
    # the file holds the sites of match_form_sites.sites(), all of them, with their inputs unchanged
    strip = [{k: v for k, v in s.items() if k not in ("expect", "compute_units")} for s in sites]
    assert strip == mfs.sites()
    assert all(s["compute_units"] == golden["compute_units"] for s in sites)
    families = set()
    for s in sites:
        assert s["expect"]["kernel"] in KERNEL_FAMILY, s
        families |= KERNEL_FAMILY[s["expect"]["kernel"]]
    assert families == set(mfs.FAMILIES)
    assert any("part-filled" in s["expect"]["kernel"] for s in sites)
    for knob in mfs.KNOBS:
        assert any(knob in s["env"] for s in sites), knob
    assert {int(s["env"]["HSM_WPS"]) for s in sites if "HSM_WPS" in s["env"]} == {1, 2, 4, 8, 16}
    assert {s["parity"] for s in sites} == {"auto", "exact", "fast", "relaxed"}
    assert {s["layout"] for s in sites} == {"quad", "plane"}
    assert {s["n"] for s in sites if s["entry"] == "batch"} >= set(mfs.BEAMS)
    assert {s["n"] for s in sites if s["entry"] == "single"} >= set(mfs.SINGLE_BEAMS)
    assert {tuple(s["batch_cu"]) for s in sites if s["entry"] == "batch"} >= set(mfs.BATCHES)
    assert {s["map"] for s in sites} == set(mfs.MAPS)
    assert any(s["probe"] for s in sites)


def test_plan_gives_the_recorded_form_at_every_site(check, golden):
    got = plans(check, golden)
    assert len(got) == len(golden["sites"])
    wrong = []
    for s, p in zip(golden["sites"], got):
        e = s["expect"]
        if (p["kernel"], p["config"], p["parity"]) != (e["kernel"], e["config"], e["parity"]) or \
                p["family"] not in KERNEL_FAMILY[e["kernel"]]:
            wrong.append((s["id"], p, e))
    assert not wrong, (len(wrong), wrong[:5])


@pytest.mark.parametrize("mode,least", [("cases", 25), ("staging", 1000000)])
def test_what_the_record_cannot_show(check, mode, least):
    r = subprocess.run([check, mode], capture_output=True, text=True)
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert r.returncode == 0 and rec["mismatches"] == 0, (rec, r.stderr[-2000:])
    assert rec["cases"] >= least, rec
