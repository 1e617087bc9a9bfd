#!/usr/bin/env python3
"""Is the device code of this tree the device code of another commit?  For changes that may touch host code only.

Compiles `hector_slam_amd.build.device_asm()` -- the gfx950 assembly of every translation unit -- for the working tree and for
`--base` (a git revision, exported to a temporary directory and compiled with ITS build.py), and compares the two texts.  The one
thing allowed to differ is the name of hipcc's per-unit `__hip_cuid_<hash>` byte, which hashes the source file as a whole, host
code and path included.  No GPU needed.  Prints one JSON line; exit status 1 when the texts differ.

usage: tools/diff_device_asm.py [--base HEAD]
"""
import argparse
import difflib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ASM = "import sys; from hector_slam_amd import build as hb; sys.stdout.write(hb.device_asm())"


def device_asm(tree: str) -> list[str]:
    text = subprocess.run([sys.executable, "-c", _ASM], cwd=tree, check=True, capture_output=True, text=True).stdout
    return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", text).splitlines()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", default="HEAD", help="the revision to compare the working tree with")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        tar = subprocess.run(["git", "-C", ROOT, "archive", args.base, "hector_slam_amd", "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", d], input=tar, check=True)
        base, mine = device_asm(d), device_asm(ROOT)
    diff = list(difflib.unified_diff(base, mine, args.base, "working tree", lineterm="", n=2))
    for line in diff[:80]:
        print(line, file=sys.stderr)
    print(json.dumps({"base": args.base, "lines": len(mine), "identical": not diff}))
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
