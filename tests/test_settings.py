"""What hsm_opts and the environment decide about a context (hector_slam_amd/csrc/settings.h: parse_settings) on the CPU.

tests/cpp/settings_check.cpp restates the chain of getenv lines hsm_create carried before the parser, on a plain bag of the
context's fields, and runs both through an injected environment: every HSM_* name over unset, the empty string, numbers and every
word a setting knows, with hsm_opts absent and with every layout and waves-per-scan value.  Every field and every refusal (code and
text) must agree."""
import json
import os
import re
import subprocess

import pytest

from support import build_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hector_slam_amd", "csrc")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return str(build_check(tmp_path_factory.mktemp("settings"), "settings_check.cpp", "-I", os.path.join(ROOT, "include")))


def test_parser_is_the_chain_it_replaced(check):
    r = subprocess.run([check], capture_output=True, text=True)
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert r.returncode == 0 and rec["mismatches"] == 0, (rec, r.stderr[-2000:])
    # 33 names x 20 values, each with hsm_opts absent and with 4 layouts x 8 widths
    assert rec["cases"] >= 33 * 20 * 33, rec


def test_the_check_knows_every_setting_the_library_reads():
    """a getenv("HSM_...") anywhere in csrc/ is one of the check's names, and the context's are read in settings.h only"""
    check_names = set(re.findall(r'"(HSM_[A-Z0-9_]+)"', open(os.path.join(ROOT, "tests", "cpp", "settings_check.cpp")).read()))
    parsed = set(re.findall(r'env\w*\(env, "(HSM_[A-Z0-9_]+)"', open(os.path.join(CSRC, "settings.h")).read()))
    assert len(parsed) == 31
    elsewhere = {}
    for f in sorted(os.listdir(CSRC)):
        for name in re.findall(r'getenv\("(HSM_[A-Z0-9_]+)"\)', open(os.path.join(CSRC, f)).read()):
            elsewhere.setdefault(f, set()).add(name)
    assert elsewhere == {"group.hip": {"HSM_GROUP_GATHER"}, "pose_exchange.hip": {"HSM_EXCHANGE_TIMEOUT_MS"}}
    assert check_names == parsed | {"HSM_GROUP_GATHER", "HSM_EXCHANGE_TIMEOUT_MS"}
