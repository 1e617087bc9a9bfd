"""The error the REFERENCE chain leaves on the end-to-end scene of tests/align_cases.py, on the CPU: the bound of
tests/test_gpu_align_map.py's end-to-end test is twice this, per component.

Both maps are built by the CPU checker (oracle/) from the scene's scans; the points are the numpy model's (tests/points_cases.py)
of src's level 0; the chain is tests/test_window_model.py's reference_relocalize on dst with the guess (0, 0, 0): likelihoods over
the window on the search level, the strict top k, a match from each start, the likelihood on level 0, the winner.  Also prints the
occupied cells of the dense pair's level 0.  No GPU.

  python tools/align_reference_error.py
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def built(pyoracle, kind, geom, scans):
    o = pyoracle.Oracle(kind, geom[0], geom[1], geom[2], geom[3], geom[4])
    o.set_update_factor_free(0.4)
    o.set_update_factor_occupied(0.9)
    o.build_map([p for p, _ in scans], [s for _, s in scans])
    return o


def main():
    import align_cases as ac
    import merge_cases as mc
    import points_cases as pc
    from conftest import oracle_kinds
    from oracle import pyoracle
    from test_window_model import reference_relocalize
    pyoracle.build()
    kind = oracle_kinds()[-1]
    dst_scans, src_scans = ac.e2e_scans()
    dst, src = built(pyoracle, kind, ac.E2E_GEOM, dst_scans), built(pyoracle, kind, ac.E2E_GEOM, src_scans)
    lo = src.download_level(0)[0]
    every = max(1, -(-len(pc.kept_cells(lo, None, 1)) // ac.MAX_POINTS))
    pts, counts = pc.occupied_points_model(lo, None, every, ac.MAX_POINTS, pc.world_from_map(ac.E2E_GEOM, 0), pc.scale_to_map(ac.E2E_GEOM))
    r = reference_relocalize(dst, types.SimpleNamespace(levels=ac.E2E_GEOM[3]), np.zeros(3, np.float32), pts, ac.STEP, ac.HALF, ac.K,
                             search_level=ac.SEARCH_LEVEL)
    err = ac.error(r["best_pose"])
    print(f"{kind}: every {every}, {counts[0]} points, winner window index {r['best_index']}, pose {r['best_pose'].tolist()}")
    print("reference error per component (m, m, rad):", [float("%.6g" % e) for e in err], " truth", ac.TRUTH)
    print("below one level-0 cell and 0.02 rad:", bool(err[0] < ac.E2E_GEOM[0] and err[1] < ac.E2E_GEOM[0] and err[2] < 0.02))
    dense = built(pyoracle, kind, ac.DENSE_GEOM, ac.dense_scans())
    print("dense pair: occupied cells of level 0:", len(pc.kept_cells(dense.download_level(0)[0], None, 1)))
    for pair, (gd, gs) in mc.PAIRS.items():
        s = built(pyoracle, kind, gs, mc.build_scans(31))
        print(pair, "pair: occupied cells of src's level 0:", len(pc.kept_cells(s.download_level(0)[0], None, 1)))


if __name__ == "__main__":
    main()
