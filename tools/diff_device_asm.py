#!/usr/bin/env python3
"""Is the device code of this tree the device code of another commit?  For changes that may touch host code only.

Compiles `hector_slam_amd.build.device_asm()` -- the gfx950 assembly of every translation unit -- for the working tree and for
`--base` (a git revision, exported to a temporary directory and compiled with ITS build.py), and compares the two texts.  The one
thing allowed to differ is the name of hipcc's per-unit `__hip_cuid_<hash>` byte, which hashes the source file as a whole, host
code and path included.  No GPU needed.  Prints one JSON line; exit status 1 when the texts differ.

--by-kernel: for changes that move kernels between translation units, where the whole texts cannot agree.  Each tree's assembly is
split at its kernel symbols, and the map from kernel name to (body, .amdhsa_* descriptor block) is compared instead: names on one
side only, and names whose text differs, are reported.  Local labels carry the number of the function within its unit
(.LBB<k>_<n>, .Lfunc_end<k>) or a running one (.Ltmp<n>); both are normalised.  A kernel that several units instantiate must
be the same text in all of them.

usage: tools/diff_device_asm.py [--base HEAD] [--by-kernel]
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


def kernels(lines: list[str], where: str, clashes: list[str]) -> dict[str, tuple[str, str]]:
    """kernel name -> (body, descriptor block), labels normalised; a name whose occurrences differ goes to `clashes`"""
    out: dict[str, tuple[str, str]] = {}
    starts: dict[str, list[int]] = {}  # every body of a name, one per unit that defines it
    for i, l in enumerate(lines):
        if m := re.match(r"(\S+):\s+; @\1$", l):
            starts.setdefault(m.group(1), []).append(i)
    for i, l in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", l)
        if not m:
            continue
        name = m.group(1)
        first = max((j for j in starts.get(name, []) if j < i), default=None)  # the nearest body in front of this descriptor
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        if first is None:
            clashes.append(f"{where}: {name} has a descriptor and no body")
            continue
        tmp: dict[str, int] = {}

        def norm(text: str) -> str:
            text = re.sub(r"\.L([A-Za-z_]+?)\d+_(\d+)", r".L\1_\2", text)
            text = re.sub(r"\bBB\d+_(\d+)", r"BB_\1", text)  # (the same number in the compiler's loop comments ...)
            text = re.sub(r"[ \t]+;", " ;", text)             # (... which it aligns behind labels of either width)
            text = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", text)
            return re.sub(r"\.Ltmp\d+", lambda t: f".Ltmp{tmp.setdefault(t.group(0), len(tmp))}", text)
        entry = (norm("\n".join(lines[first:i])), norm("\n".join(lines[i:end + 1])))
        if out.setdefault(name, entry) != entry:
            clashes.append(f"{where}: {name} differs between two units")
    return out


def by_kernel(base: list[str], mine: list[str], base_name: str) -> int:
    clashes: list[str] = []
    kb, km = kernels(base, base_name, clashes), kernels(mine, "working tree", clashes)
    only_base, only_mine = sorted(set(kb) - set(km)), sorted(set(km) - set(kb))
    differ = sorted(n for n in set(kb) & set(km) if kb[n] != km[n])
    for what, names in (("only in " + base_name, only_base), ("only in the working tree", only_mine), ("text differs", differ)):
        for n in names:
            print(f"{what}: {n}", file=sys.stderr)
    for c in clashes:
        print(c, file=sys.stderr)
    for n in differ[:3]:
        for part in (0, 1):
            for line in list(difflib.unified_diff(kb[n][part].splitlines(), km[n][part].splitlines(), base_name, "working tree", lineterm="", n=2))[:40]:
                print(line, file=sys.stderr)
    same = not (only_base or only_mine or differ or clashes)
    print(json.dumps({"base": base_name, "kernels": len(km), "only_base": len(only_base), "only_working_tree": len(only_mine),
                      "differ": len(differ), "clashes": len(clashes), "identical": same}))
    return 0 if same else 1


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", default="HEAD", help="the revision to compare the working tree with")
    ap.add_argument("--by-kernel", action="store_true", help="compare kernel by kernel (kernels may have changed units)")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        tar = subprocess.run(["git", "-C", ROOT, "archive", args.base, "hector_slam_amd", "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", d], input=tar, check=True)
        base, mine = device_asm(d), device_asm(ROOT)
    if args.by_kernel:
        return by_kernel(base, mine, args.base)
    diff = list(difflib.unified_diff(base, mine, args.base, "working tree", lineterm="", n=2))
    for line in diff[:80]:
        print(line, file=sys.stderr)
    print(json.dumps({"base": args.base, "lines": len(mine), "identical": not diff}))
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
