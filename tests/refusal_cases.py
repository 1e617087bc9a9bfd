"""The refusals of the host runtime's scan-log, update and raw-scan entries, as a list of named cases: an entry of the C ABI plus
arguments that make it refuse before anything is queued.  tests/tools/record_host_refusals.py ran them on the commit before the
entries were rewritten onto argument bundles and wrote tests/golden/host_refusals.json (status code and the full hsm_last_error()
text of every case); tests/test_gpu_host_refusals.py replays them against the library under test and compares both exactly -- which
check wins where two apply, and the entry name in every text, are what such a rewrite can change silently.

Arguments are symbolic so that no address reaches the golden file: "D" a device buffer, "D+4" the same at an address 4 mod 8,
"D+1" at an odd one, "H" a host array, "S" the test's stream, None a null pointer.  No pointer is ever dereferenced: every case
refuses first.  Cases with capture=True run while "S" is being captured into a graph.

The probes, downloads, test hooks and the device group joined the list before they moved out of the core translation unit (recorded
again, all cases, from the commit before that move).  Their first argument is the context unless FIRST says otherwise; the override
`ctx=None` passes a null context (or group) instead.

The single-scan conversions (INGEST) and one failing HIP status check joined it before raw-scan conversion and the occupancy
exports moved to ingest.hip and occupancy.hip (recorded again, all cases, from the commit before that move).

The batched match, score, covariance, select and chain entries, the window and relocalisation entries and the device readers of
rays.hip (MATCHER) joined it before the matcher's front door was rewritten onto argument bundles and every map reader onto one
bracket (recorded again, all cases, from the commit before that rewrite).  Like the MOVED entries they are called through bare
addresses.  The steps and half-extents of a window are host arrays the entry reads: "H_STEP", "H_HALF" and their bad variants.
"""
INT_MAX = 2**31 - 1
MAX_BEAMS = 1048575  # HSM_MAX_UPDATE_BEAMS
N = 8                # beams of the raw-scan entries' default call
COUNT = 2

_TF = [("angle_min", -1.0), ("angle_increment", 0.25), ("range_min", 0.1), ("range_max", 30.0), ("range_cutoff", -1.0)]
_GATES = [("sqr_laser_min_dist", 0.01), ("sqr_laser_max_dist", 900.0), ("laser_z_min", -1.0), ("laser_z_max", 1.0), ("scale_to_map", 20.0)]

# entry -> its parameters behind the context, in ABI order, with the value of a call that would be accepted
ENTRIES = {
    "hsm_update_by_scans_device": [("count", COUNT), ("poses", "D"), ("pts", "D"), ("offsets", "D"), ("shared_n", 0), ("max_beams", 0),
                                   ("origo", None), ("stream", "S")],
    "hsm_update_by_scans_device_origos": [("count", COUNT), ("poses", "D"), ("pts", "D"), ("offsets", "D"), ("shared_n", 0),
                                          ("max_beams", 0), ("origos", "D"), ("stream", "S")],
    "hsm_update_by_scans_device_gated": [("count", COUNT), ("poses", "D"), ("pts", "D"), ("offsets", "D"), ("shared_n", 0),
                                         ("max_beams", 0), ("origo", None), ("force", None), ("out_applied", None), ("stream", "S")],
    "hsm_update_by_scans_device_gated_origos": [("count", COUNT), ("poses", "D"), ("pts", "D"), ("offsets", "D"), ("shared_n", 0),
                                                ("max_beams", 0), ("origos", "D"), ("force", None), ("out_applied", None),
                                                ("stream", "S")],
    "hsm_slam_scans_device": [("count", COUNT), ("start_pose", "D"), ("hint_deltas", None), ("pts", "D"), ("offsets", "D"),
                              ("max_beams", 0), ("origo", None), ("force", None), ("out_pose", "D"), ("out_cov", None),
                              ("out_applied", None), ("stream", "S")],
    "hsm_slam_scans_device_origos": [("count", COUNT), ("start_pose", "D"), ("hint_deltas", None), ("pts", "D"), ("offsets", "D"),
                                     ("max_beams", 0), ("origos", "D"), ("force", None), ("out_pose", "D"), ("out_cov", None),
                                     ("out_applied", None), ("stream", "S")],
    "hsm_update_by_scans": [("count", COUNT), ("poses", "H"), ("pts", "H"), ("offsets", None), ("shared_n", N), ("origo", None)],
    "hsm_match_batch_ranges": [("batch", COUNT), ("begin", "H"), ("ranges", "H"), ("n", N)] + _TF[:4] + [("scale_to_map", 20.0),
                               ("out_pose", "H"), ("out_cov", None), ("out_counts", None)],
    "hsm_match_batch_ranges_device": [("batch", COUNT), ("begin", "D"), ("ranges", "D"), ("n", N)] + _TF[:4] + [
        ("scale_to_map", 20.0), ("out_pose", "D"), ("out_cov", None), ("out_counts", None), ("workspace", "D"),
        ("workspace_bytes", "WS_RANGES"), ("stream", "S")],
    "hsm_ingest_batch_ranges_tf_device": [("batch", COUNT), ("ranges", "D"), ("n", N)] + _TF + [("tf_rows", "D"), ("shared_tf", 0)] +
                                         _GATES + [("out_pts", "D"), ("out_offsets", "D"), ("out_counts", "D"), ("out_origo", None),
                                                   ("stream", "S")],
    "hsm_match_batch_ranges_tf": [("batch", COUNT), ("begin", "H"), ("ranges", "H"), ("n", N)] + _TF + [("tf_rows", "H"),
                                  ("shared_tf", 0)] + _GATES + [("out_pose", "H"), ("out_cov", None), ("out_counts", None),
                                                                ("out_origo", None)],
    "hsm_slam_ranges_tf_device": [("count", COUNT), ("start_pose", "D"), ("hint_deltas", None), ("ranges", "D"), ("n", N)] + _TF +
                                 [("tf_rows", "D"), ("shared_tf", 0)] + _GATES + [("force", None), ("out_pose", "D"), ("out_cov", None),
                                  ("out_applied", None), ("out_counts", None), ("workspace", "D"), ("workspace_bytes", "WS_SLAM"),
                                  ("stream", "S")],
    "hsm_slam_ranges_tf": [("count", COUNT), ("start_pose", "H"), ("hint_deltas", None), ("ranges", "H"), ("n", N)] + _TF +
                          [("tf_rows", "H"), ("shared_tf", 0)] + _GATES + [("force", None), ("out_pose", "H"), ("out_cov", None),
                           ("out_applied", None), ("out_counts", None), ("out_origo", None)],
}

# the entries that moved to probes.hip and group.hip
_STATES = [("level", 0), ("batch", COUNT), ("states", "H"), ("pts", "H"), ("n", N)]
_POSE_PTS = [("level", 0), ("pose", "H"), ("pts", "H"), ("n", N)]
MOVED = {
    "hsm_likelihood_states": _STATES + [("out", "H")],
    "hsm_residual_states": _STATES + [("out", "H")],
    "hsm_covariance_for_poses": _STATES + [("out_cov_map", "H"), ("out_cov_world", None), ("out_lh7", None)],
    "hsm_ray_distances": [("level", 0), ("origin_x", 0.0), ("origin_y", 0.0), ("resolution", 0.05), ("n", N), ("begin", "H"),
                          ("end", "H"), ("out_dist", "H"), ("out_hit", None)],
    "hsm_hessian_derivs": _POSE_PTS + [("H", "H"), ("dTr", "H")],
    "hsm_eval_beams": _POSE_PTS + [("out4", "H")],
    "hsm_level_info": [("level", 0), ("sx", None), ("sy", None), ("cell", None), ("scale", None)],
    "hsm_map_coords_pose": [("level", 0), ("w", "H"), ("m", "H")],
    "hsm_world_coords_pose": [("level", 0), ("m", "H"), ("w", "H")],
    "hsm_update_index": [("level", 0)],
    "hsm_download_level": [("level", 0), ("logodds", None), ("update_index", None)],
    "hsm_upload_level": [("level", 0), ("logodds", None), ("update_index", None)],
    "hsm_download_rows": [("level", 0), ("y0", 0), ("y1", 1), ("rows", "H")],
    "hsm_download_cells": [("level", 0), ("x0", 0), ("y0", 0), ("x1", 1), ("y1", 1), ("dst", "H"), ("pitch", 2)],
    "hsm_last_update_bbox": [("level", 0), ("bbox", "H")],
    "hsm_take_dirty_bbox": [("level", 0), ("bbox", "H")],
    "hsm_download_prob": [("level", 0), ("prob", "H")],
    "hsm_debug_set_coop_barrier": [("value", 0)],
    "hsm_debug_set_coop_mute": [("block_plus_one", 0)],
    "hsm_debug_set_schedule": [("level", -1), ("gn_steps", 0)],
    "hsm_debug_batch_order": [("batch", COUNT), ("begin", "D"), ("perm", "D"), ("stream", "S")],
    "hsm_debug_spec_stats": [("enable", 0), ("out", None)],
    "hsm_debug_marks_nonzero": [("level", 0), ("out", "H")],
    "hsm_debug_set_update_serial": [("level", 0), ("serial", 1)],
    "hsm_debug_expf": [("n", N), ("x", "H"), ("out_a", "H"), ("out_b", "H")],
    "hsm_debug_sincos": [("n", N), ("x", "H"), ("out_a", "H"), ("out_b", "H")],
    "hsm_group_create": [("map_resolution", 0.05), ("size_x", 64), ("size_y", 64), ("levels", 1), ("start_x", 0.5), ("start_y", 0.5),
                         ("devices", "H_ZERO_INT"), ("n_devices", 1), ("out", "H")],
    "hsm_group_set_gather": [("mode", 0)],
    "hsm_group_debug_force_p2p": [("on", 0)],
    "hsm_group_set_update_factors": [("free", 0.4), ("occupied", 0.9)],
    "hsm_group_process_scan": [("hint", "H"), ("pts", "H"), ("n", N), ("origo", None), ("do_update", 0), ("out_pose", "H"), ("cov", "H")],
    "hsm_group_match_batch_device": [("counts", "H_ONE_INT"), ("begin", "H_PTR_D"), ("pts", "H_PTR_D"), ("offsets", None), ("shared_n", N),
                                     ("root", 0), ("out_pose_all", "D"), ("out_cov_all", None)],
    "hsm_group_synchronize": [],
    "hsm_group_match_batch": [("batch", COUNT), ("begin", "H"), ("pts", "H"), ("offsets", None), ("shared_n", N), ("out_pose", "H"),
                              ("out_cov", None)],
    "hsm_shard_bounds": [("total", 10), ("rank", 0), ("world", 2), ("begin", "H"), ("end", "H")],
}
# the single-scan conversions, which joined the list before they moved to ingest.hip
INGEST = {
    "hsm_ingest_laser_scan": [("ranges", "H"), ("n", N)] + _TF[:4] + [("scale_to_map", 20.0), ("out_pts", None), ("out_n", None)],
    "hsm_ingest_laser_scan_tf": [("ranges", "H"), ("n", N)] + _TF + [("tf_rows", "H")] + _GATES + [("out_pts", None), ("out_n", None),
                                                                                                 ("out_origo", None)],
}
# the matcher's front door (match.hip), the window entries (window.hip) and the device readers of rays.hip
_SCANS = [("pts", "D"), ("offsets", None), ("shared_n", N)]
_MATCH = [("batch", COUNT), ("begin", "D")] + _SCANS + [("out_pose", "D"), ("out_cov", None)]
_RANKING = [("groups", 0), ("group_offsets", None), ("group_size", 0), ("out_index", None), ("out_score", None), ("out_best_pose", None)]
_COV_OUT = [("out_cov_world", "D"), ("out_cov_map", None), ("out_lh7", None), ("out_likelihood", "D")]
_WINDOW = [("center", "D"), ("step", "H_STEP"), ("half", "H_HALF")]
_HOST = lambda params: [(k, "H" if v == "D" else v) for k, v in params]  # noqa: E731
MATCHER = {
    "hsm_match_batch_device": _MATCH + [("stream", "S")],
    "hsm_match_batch_device_gather": _MATCH + [("exchange", "D"), ("first_row", 0), ("lag", 0), ("out_all", None), ("stream", "S")],
    "hsm_score_batch_device": [("level", 0), ("batch", COUNT), ("poses", "D")] + _SCANS + [("out_likelihood", "D"), ("out_residual", None),
                                                                                           ("stream", "S")],
    "hsm_covariance_batch_device": [("level", 0), ("batch", COUNT), ("poses", "D")] + _SCANS + _COV_OUT + [("stream", "S")],
    "hsm_select_best_device": [("groups", 1), ("group_offsets", None), ("group_size", COUNT), ("scores", "D"), ("poses", "D"),
                               ("out_index", "D"), ("out_score", None), ("out_pose", None), ("stream", "S")],
    "hsm_match_score_batch_device": _MATCH + [("level", 0), ("out_likelihood", "D"), ("out_residual", None)] + _RANKING + [("stream", "S")],
    "hsm_match_cov_batch_device": _MATCH + [("level", 0)] + _COV_OUT + _RANKING + [("stream", "S")],
    "hsm_match_batch": _HOST(_MATCH),
    "hsm_match_score_batch": _HOST(_MATCH) + [("level", 0), ("out_likelihood", "H"), ("out_residual", None)] + _RANKING,
    "hsm_covariance_batch": [("level", 0), ("batch", COUNT), ("poses", "H")] + _HOST(_SCANS) + _HOST(_COV_OUT),
    "hsm_score_window_device": [("level", 0)] + _WINDOW + [("pts", "D"), ("n", N), ("out_likelihood", "D"), ("out_residual", None),
                                                           ("stream", "S")],
    "hsm_relocalize_device": [("level", 0)] + _WINDOW + [("k", 2), ("pts", "D"), ("n", N), ("workspace", "D"),
                                                         ("workspace_bytes", "WS_RELOC"), ("cand_pose", "D"), ("cand_cov", None),
                                                         ("cand_likelihood", "D"), ("best_pose", "D"), ("best_score", None),
                                                         ("best_index", "D"), ("stream", "S")],
    "hsm_ray_distances_device": [("level", 0), ("origin_x", 0.0), ("origin_y", 0.0), ("resolution", 0.05), ("n", N), ("begin", "D"),
                                 ("end", "D"), ("out_dist", "D"), ("out_hit", None), ("stream", "S")],
    "hsm_cast_scans_device": [("level", 0), ("batch", COUNT), ("poses", "D"), ("angles", "D"), ("n", N), ("range_max", 30.0),
                              ("out_ranges", "D"), ("out_hit", None), ("stream", "S")],
    "hsm_occupied_points_device": [("level", 0), ("bbox", None), ("every", 1), ("max_points", N), ("out_pts", "D"), ("out_count", "D"),
                                   ("workspace", "D"), ("workspace_bytes", "WS_POINTS"), ("stream", "S")],
}
_CHAINS = ["hsm_match_score_batch_device", "hsm_match_cov_batch_device"]
_BATCH_READERS = ["hsm_score_batch_device", "hsm_covariance_batch_device", "hsm_covariance_batch"]
_WINDOWS = ["hsm_score_window_device", "hsm_relocalize_device"]
# what goes in front of an entry's parameters: the context (every entry not listed), the runner's one-device group, or nothing
FIRST = {e: "group" for e in MOVED if e.startswith("hsm_group_")}
FIRST.update({"hsm_group_create": None, "hsm_shard_bounds": None})
_LEVELLED = [e for e, params in MOVED.items() if params and params[0][0] == "level" and e != "hsm_debug_set_schedule"]

_UPDATES = [e for e in ENTRIES if e.startswith("hsm_update_by_scans_device")]
_SLAM_SCANS = ["hsm_slam_scans_device", "hsm_slam_scans_device_origos"]
_RANGES = ["hsm_match_batch_ranges", "hsm_match_batch_ranges_device"]
_TF_ENTRIES = ["hsm_ingest_batch_ranges_tf_device", "hsm_match_batch_ranges_tf", "hsm_slam_ranges_tf_device", "hsm_slam_ranges_tf"]
_ORIGOS = [e for e in ENTRIES if e.endswith("origos")]
_UNSEEN = {"angle_min": -0.875, "angle_increment": 0.125}  # a sensor geometry no other case or test uses


def _count_name(entry):
    return "batch" if "batch" in ENTRIES[entry][0][0] else "count"


def cases():
    """[(name, entry, overrides, capture)]"""
    out = []

    def add(what, entry, capture=False, **over):
        out.append((f"{entry}:{what}", entry, over, capture))

    for e in ENTRIES:
        if e not in MOVED and e not in INGEST and e not in MATCHER:
            add("negative count", e, **{_count_name(e): -1})
    for e in _UPDATES + _SLAM_SCANS:
        add("negative max_beams", e, max_beams=-5)
    for e in _RANGES + _TF_ENTRIES:
        add("negative n", e, n=-1)
        add("n above HSM_MAX_UPDATE_BEAMS", e, n=MAX_BEAMS + 1)
        add("count * n above INT_MAX", e, **{_count_name(e): 2049, "n": MAX_BEAMS})  # 2049 * 1048575 = INT_MAX + 1 + 1048576 - 2049
        add("null ranges", e, ranges=None)
    for e in _UPDATES + ["hsm_update_by_scans"]:
        add("null poses", e, poses=None)
        add("null pts for a shared scan", e, pts=None, offsets=None, shared_n=100)
        add("negative shared_n without offsets", e, offsets=None, shared_n=-1)
        add("shared_n above HSM_MAX_UPDATE_BEAMS", e, offsets=None, shared_n=MAX_BEAMS + 1)
    for e in _ORIGOS:
        add("origos at 4 mod 8", e, origos="D+4")
    for e in ["hsm_ingest_batch_ranges_tf_device", "hsm_slam_ranges_tf_device"]:
        add("tf_rows at 4 mod 8", e, tf_rows="D+4")
    for e in _TF_ENTRIES:
        add("null tf_rows", e, tf_rows=None)
    for e, ws in (("hsm_match_batch_ranges_device", "WS_RANGES"), ("hsm_slam_ranges_tf_device", "WS_SLAM")):
        add("null workspace", e, workspace=None)
        add("workspace one byte short", e, workspace_bytes=ws + "-1")
        add("workspace at an odd address", e, workspace="D+1")
    add("offsets that decrease", "hsm_update_by_scans", offsets="H_DECREASING", shared_n=0)
    add("offsets that start below zero", "hsm_update_by_scans", offsets="H_NEGATIVE", shared_n=0)
    for e in _SLAM_SCANS + _RANGES + ["hsm_match_batch_ranges_tf", "hsm_slam_ranges_tf_device", "hsm_slam_ranges_tf"]:
        add("null output pose", e, out_pose=None)
    for e in _SLAM_SCANS:
        add("null offsets", e, offsets=None)
    for e in ["hsm_match_batch_ranges", "hsm_match_batch_ranges_device", "hsm_match_batch_ranges_tf"]:
        add("null start poses", e, begin=None)
    add("null outputs", "hsm_ingest_batch_ranges_tf_device", out_pts=None)
    # two refusals at once: which one the caller hears
    add("negative count and too many beams", "hsm_update_by_scans_device", count=-1, offsets=None, shared_n=MAX_BEAMS + 1)
    add("too many beams and a null workspace", "hsm_slam_ranges_tf_device", n=MAX_BEAMS + 1, workspace=None)
    add("misaligned tf_rows and too many beams", "hsm_slam_ranges_tf_device", tf_rows="D+4", n=MAX_BEAMS + 1)
    add("misaligned origos and a negative count", "hsm_slam_scans_device_origos", origos="D+4", count=-1)
    add("null pts and decreasing offsets", "hsm_update_by_scans", pts=None, offsets="H_DECREASING", shared_n=0)
    # while "S" is being captured into a graph
    for e in _UPDATES + _SLAM_SCANS + ["hsm_slam_ranges_tf_device"]:
        add("stream under capture", e, capture=True)
    for e in ["hsm_match_batch_ranges_device", "hsm_ingest_batch_ranges_tf_device"]:
        add("unseen geometry under capture", e, capture=True, **_UNSEEN)
    add("too many beams under capture", "hsm_update_by_scans_device", capture=True, offsets=None, shared_n=MAX_BEAMS + 1)
    add("short workspace under capture", "hsm_slam_ranges_tf_device", capture=True, workspace_bytes="WS_SLAM-1")
    moved_cases(add)
    matcher_cases(add)
    for e in INGEST:
        add("null context", e, ctx=None)
        add("negative n", e, n=-1)
        add("n above HSM_MAX_UPDATE_BEAMS", e, n=MAX_BEAMS + 1)
        add("null ranges", e, ranges=None)
    add("null tf_rows", "hsm_ingest_laser_scan_tf", tf_rows=None)
    # The text of a failing HIP status check ("<the call as written>: <HIP's text>"), without a failing device: HIP keeps a thread's
    # last failure until somebody asks for it, so a call of the CALLER's that HIP refused (an invalid device ordinal) is what the
    # entry's launch check reports.  The one case that queues work: the conversion of an empty scan, which writes its count of 0.
    add("launch check behind a failed HIP call of the caller's", "hsm_ingest_laser_scan", n=0, failed_hip_call_first=True)
    assert len({c[0] for c in out}) == len(out)
    return out


def moved_cases(add):
    """the refusals of the entries in MOVED: a null context, a level out of range, negative counts, each required pointer null"""
    for e in MOVED:
        if FIRST.get(e, "ctx"):
            add("null context", e, ctx=None)
    for e in _LEVELLED:
        add("level below zero", e, level=-1)
        add("level past the pyramid", e, level=2)
    for e in ["hsm_likelihood_states", "hsm_residual_states", "hsm_covariance_for_poses"]:
        add("negative batch", e, batch=-1)
        add("negative n", e, n=-1)
        add("null states", e, states=None)
        add("null pts", e, pts=None)
        add("no output", e, **{k: None for k, _ in MOVED[e] if k.startswith("out")})
        add("negative batch and a level out of range", e, batch=-1, level=7)
    add("negative n", "hsm_ray_distances", n=-1)
    add("null begin", "hsm_ray_distances", begin=None)
    add("null end", "hsm_ray_distances", end=None)
    add("null out_dist", "hsm_ray_distances", out_dist=None)
    add("resolution zero", "hsm_ray_distances", resolution=0.0)
    add("resolution negative", "hsm_ray_distances", resolution=-0.05)
    add("resolution NaN", "hsm_ray_distances", resolution=float("nan"))
    for e in ["hsm_hessian_derivs", "hsm_eval_beams"]:
        add("null pose", e, pose=None)
        add("negative n", e, n=-1)
        add("null pts", e, pts=None)
    add("null H", "hsm_hessian_derivs", H=None)
    add("null dTr", "hsm_hessian_derivs", dTr=None)
    add("null out4", "hsm_eval_beams", out4=None)
    add("negative first row", "hsm_download_rows", y0=-1)
    add("last row past the map", "hsm_download_rows", y1=257)
    add("rows that decrease", "hsm_download_rows", y0=2, y1=1)
    add("null rows", "hsm_download_rows", rows=None)
    add("negative corner", "hsm_download_cells", x0=-1)
    add("corner past the map", "hsm_download_cells", y1=256)
    add("corners that decrease", "hsm_download_cells", x0=2, x1=1)
    add("null destination", "hsm_download_cells", dst=None)
    add("pitch below the width", "hsm_download_cells", pitch=1)
    add("null bbox", "hsm_take_dirty_bbox", bbox=None)
    add("level past the pyramid", "hsm_debug_set_schedule", level=2, gn_steps=1)
    add("no steps", "hsm_debug_set_schedule", level=0, gn_steps=0)
    add("empty batch", "hsm_debug_batch_order", batch=0)
    add("null start poses", "hsm_debug_batch_order", begin=None)
    add("null permutation", "hsm_debug_batch_order", perm=None)
    add("null out", "hsm_debug_marks_nonzero", out=None)
    add("serial past the key generation field", "hsm_debug_set_update_serial", serial=4096)
    for e in ["hsm_debug_expf", "hsm_debug_sincos"]:
        add("negative n", e, n=-1)
        add("null x", e, x=None)
        add("null first output", e, out_a=None)
        add("null second output", e, out_b=None)
    add("null out", "hsm_group_create", out=None)
    add("null devices", "hsm_group_create", devices=None)
    add("no devices", "hsm_group_create", n_devices=0)
    add("unknown mode", "hsm_group_set_gather", mode=17)
    add("null counts", "hsm_group_match_batch_device", counts=None)
    add("null start poses", "hsm_group_match_batch_device", begin=None)
    add("null pts", "hsm_group_match_batch_device", pts=None)
    add("null output", "hsm_group_match_batch_device", out_pose_all=None)
    add("root below zero", "hsm_group_match_batch_device", root=-1)
    add("root past the group", "hsm_group_match_batch_device", root=1)
    add("negative shard", "hsm_group_match_batch_device", counts="H_NEGATIVE")
    add("shard without start poses", "hsm_group_match_batch_device", begin="H_PTR_NULL")
    add("shard without pts", "hsm_group_match_batch_device", pts="H_PTR_NULL")
    add("negative batch", "hsm_group_match_batch", batch=-1)
    add("null start poses", "hsm_group_match_batch", begin=None)
    add("null output pose", "hsm_group_match_batch", out_pose=None)
    add("negative total", "hsm_shard_bounds", total=-1)
    add("no ranks", "hsm_shard_bounds", world=0)
    add("rank below zero", "hsm_shard_bounds", rank=-1)
    add("rank past the world", "hsm_shard_bounds", rank=2)
    add("null begin", "hsm_shard_bounds", begin=None)
    add("null end", "hsm_shard_bounds", end=None)


def matcher_cases(add):
    """the refusals of the entries in MATCHER"""
    no_out = lambda e: {k: None for k, _ in MATCHER[e] if k.startswith("out_") and k not in ("out_pose", "out_cov")}  # noqa: E731
    for e in MATCHER:
        add("null context", e, ctx=None)
        if MATCHER[e][0][0] == "level" or e in _CHAINS + ["hsm_match_score_batch"]:
            add("level below zero", e, level=-1)
            add("level past the pyramid", e, level=2)
    # the batch of (pose, scan) pairs
    for e in MATCHER:
        if any(k == "batch" for k, _ in MATCHER[e]):
            add("negative batch", e, batch=-1)
    for e in ["hsm_match_batch_device", "hsm_match_batch", "hsm_match_score_batch"] + _CHAINS:
        add("null start poses", e, begin=None)
        add("null output pose", e, out_pose=None)
    for e in _BATCH_READERS:
        add("null poses", e, poses=None)
    for e in ["hsm_match_batch_device"] + _CHAINS + _BATCH_READERS:
        add("negative shared_n without offsets", e, shared_n=-1)
    for e in ["hsm_match_batch", "hsm_match_score_batch"] + _CHAINS + _BATCH_READERS:
        add("null pts for a shared scan", e, pts=None, shared_n=100)
    for e in _CHAINS + _BATCH_READERS:
        add("no output", e, **no_out(e))
    add("no likelihood output", "hsm_match_score_batch", out_likelihood=None, out_residual="H")
    add("null exchange", "hsm_match_batch_device_gather", exchange=None)
    add("empty batch", "hsm_match_batch_device_gather", batch=0)
    add("null exchange and a negative batch", "hsm_match_batch_device_gather", exchange=None, batch=-1)
    add("offsets that do not start at zero", "hsm_covariance_batch", offsets="H_NEGATIVE", shared_n=0)
    add("offsets that decrease", "hsm_covariance_batch", offsets="H_DECREASING", shared_n=0)
    # the ranking
    for e in _CHAINS + ["hsm_match_score_batch"]:
        d = "H" if e == "hsm_match_score_batch" else "D"
        add("negative groups", e, groups=-1, group_size=1, out_index=d)
        add("groups without out_index", e, groups=1, group_size=COUNT)
        add("groups times group_size above the batch", e, groups=1, group_size=COUNT + 1, out_index=d)
        add("negative group_size", e, groups=1, group_size=-1, out_index=d)
        add("bad ranking and a null start pose", e, groups=1, group_size=COUNT + 1, out_index=d, begin=None)
        add("level out of range and a negative batch", e, level=7, batch=-1)
    add("groups without likelihood output", "hsm_match_score_batch_device", groups=1, group_size=COUNT, out_index="D",
        out_likelihood=None, out_residual="D")
    add("groups without likelihood output", "hsm_match_cov_batch_device", groups=1, group_size=COUNT, out_index="D", out_likelihood=None)
    add("group offsets that decrease", "hsm_match_score_batch", groups=2, group_offsets="H_GROUPS_DECREASING", out_index="H")
    add("group offsets that pass the batch", "hsm_match_score_batch", groups=2, group_offsets="H_GROUPS_PAST", out_index="H")
    add("group offsets that start below zero", "hsm_match_score_batch", groups=2, group_offsets="H_NEGATIVE", out_index="H")
    for e in _BATCH_READERS + ["hsm_cast_scans_device"]:
        add("level out of range and a negative batch", e, level=7, batch=-1)
    add("negative groups", "hsm_select_best_device", groups=-1)
    add("negative group_size", "hsm_select_best_device", group_size=-1)
    add("null out_index", "hsm_select_best_device", out_index=None)
    add("null scores", "hsm_select_best_device", scores=None)
    add("winner poses without poses", "hsm_select_best_device", poses=None, out_pose="D")
    add("groups times group_size above INT_MAX", "hsm_select_best_device", groups=65536, group_size=65536)
    # the windows
    for e in _WINDOWS:
        add("null centre", e, center=None)
        add("null steps", e, step=None)
        add("null half-extents", e, half=None)
        add("negative half-extent", e, half="H_HALF_NEGATIVE")
        add("non-finite step", e, step="H_STEP_NAN")
        add("more than INT_MAX hypotheses", e, half="H_HALF_HUGE")
        add("negative n", e, n=-1)
        add("null pts", e, pts=None)
        add("negative half-extent and a level out of range", e, half="H_HALF_NEGATIVE", level=7)
        add("negative half-extent and a negative n", e, half="H_HALF_NEGATIVE", n=-1)
    add("no output", "hsm_score_window_device", out_likelihood=None)
    add("k below one", "hsm_relocalize_device", k=0)
    add("k above HSM_MAX_TOPK", "hsm_relocalize_device", k=65)
    for k in ("cand_pose", "cand_likelihood", "best_pose", "best_index"):
        add(f"null {k}", "hsm_relocalize_device", **{k: None})
    for e, ws in (("hsm_relocalize_device", "WS_RELOC"), ("hsm_occupied_points_device", "WS_POINTS")):
        add("null workspace", e, workspace=None)
        add("workspace one byte short", e, workspace_bytes=ws + "-1")
        add("workspace at 4 mod 8", e, workspace="D+4")
    add("null best_index and a null workspace", "hsm_relocalize_device", best_index=None, workspace=None)
    # the readers of rays.hip
    add("negative n", "hsm_ray_distances_device", n=-1)
    add("null begin", "hsm_ray_distances_device", begin=None)
    add("null end", "hsm_ray_distances_device", end=None)
    add("null out_dist", "hsm_ray_distances_device", out_dist=None)
    add("resolution zero", "hsm_ray_distances_device", resolution=0.0)
    add("resolution NaN", "hsm_ray_distances_device", resolution=float("nan"))
    add("level out of range and a negative n", "hsm_ray_distances_device", level=7, n=-1)
    add("negative n", "hsm_cast_scans_device", n=-1)
    add("negative range_max", "hsm_cast_scans_device", range_max=-1.0)
    add("range_max NaN", "hsm_cast_scans_device", range_max=float("nan"))
    add("batch times n above INT_MAX", "hsm_cast_scans_device", batch=65536, n=65536)
    add("null poses", "hsm_cast_scans_device", poses=None)
    add("null angles", "hsm_cast_scans_device", angles=None)
    add("null ranges", "hsm_cast_scans_device", out_ranges=None)
    add("negative batch and null poses", "hsm_cast_scans_device", batch=-1, poses=None)
    # a level's occupied cells
    add("every below one", "hsm_occupied_points_device", every=0)
    add("negative max_points", "hsm_occupied_points_device", max_points=-1)
    add("null counts", "hsm_occupied_points_device", out_count=None)
    add("null points", "hsm_occupied_points_device", out_pts=None)
    add("every below one and a level out of range", "hsm_occupied_points_device", every=0, level=7)
    add("negative max_points and a null workspace", "hsm_occupied_points_device", max_points=-1, workspace=None)


ENTRIES.update(MOVED)
ENTRIES.update(INGEST)
ENTRIES.update(MATCHER)


class Runner:
    """runs cases on one context: the smallest pyramid the refusal tests use, an empty map, no scan data"""

    def __init__(self, capi):
        import numpy as np
        import torch
        self.torch = torch
        self.lib = capi.load_library()
        self.g = capi.MapRepMultiMap(0.05, 256, 256, 2)
        self.dev = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda:0")
        self.host = np.zeros(1 << 12, np.float32)
        self.decreasing = np.int32([0, 50, 20])
        self.negative = np.int32([-1, 4, 8])
        self.stream = torch.cuda.Stream()
        assert self.dev.data_ptr() % 256 == 0
        # the moved entries: every array argument as a bare address (the binding's array types take no null), and a group of one device
        import ctypes as C
        self.raw = C.CDLL(self.lib._name)
        for entry in list(MOVED) + list(MATCHER):
            restype, argtypes = capi.SIGNATURES[entry]
            fn = getattr(self.raw, entry)
            fn.restype, fn.argtypes = restype, [a if a in (C.c_int, C.c_uint, C.c_float, C.c_size_t) else C.c_void_p for a in argtypes]
        self.zero_int, self.one_int = np.int32([0]), np.int32([1])
        self.ptr_d, self.ptr_null = np.uint64([self.dev.data_ptr()]), np.uint64([0])
        self.step, self.step_nan = np.float32([0.05, 0.05, 0.01]), np.float32([0.05, np.nan, 0.01])
        self.half, self.half_negative, self.half_huge = np.int32([1, 1, 0]), np.int32([1, -1, 0]), np.int32([1000, 1000, 1000])
        self.groups_decreasing, self.groups_past = np.int32([0, 2, 1]), np.int32([0, 1, 3])
        self.group = C.c_void_p()
        assert self.lib.hsm_group_create(0.05, 64, 64, 1, 0.5, 0.5, self.zero_int, 1, C.byref(self.group)) == 0
        self.values = {
            "D": self.dev.data_ptr(), "D+4": self.dev.data_ptr() + 4, "D+1": self.dev.data_ptr() + 1, "H": self.host.ctypes.data,
            "H_DECREASING": self.decreasing.ctypes.data, "H_NEGATIVE": self.negative.ctypes.data, "S": self.stream.cuda_stream,
            "WS_RANGES": int(self.lib.hsm_match_batch_ranges_workspace(COUNT, N)),
            "WS_SLAM": int(self.lib.hsm_slam_ranges_tf_workspace(COUNT, N)),
            "H_ZERO_INT": self.zero_int.ctypes.data, "H_ONE_INT": self.one_int.ctypes.data, "H_PTR_D": self.ptr_d.ctypes.data,
            "H_PTR_NULL": self.ptr_null.ctypes.data,
            "H_STEP": self.step.ctypes.data, "H_STEP_NAN": self.step_nan.ctypes.data, "H_HALF": self.half.ctypes.data,
            "H_HALF_NEGATIVE": self.half_negative.ctypes.data, "H_HALF_HUGE": self.half_huge.ctypes.data,
            "H_GROUPS_DECREASING": self.groups_decreasing.ctypes.data, "H_GROUPS_PAST": self.groups_past.ctypes.data,
            "WS_RELOC": int(self.lib.hsm_relocalize_workspace(9, 2)),      # the 3 x 3 x 1 window of H_HALF, k = 2
            "WS_POINTS": int(self.lib.hsm_occupied_points_workspace(256 * 256)),  # level 0, whole
        }
        self.values["WS_RANGES-1"] = self.values["WS_RANGES"] - 1
        self.values["WS_SLAM-1"] = self.values["WS_SLAM"] - 1
        self.values["WS_RELOC-1"] = self.values["WS_RELOC"] - 1
        self.values["WS_POINTS-1"] = self.values["WS_POINTS"] - 1
        assert 0 < self.values["WS_RELOC"] <= self.dev.numel() and 0 < self.values["WS_POINTS"] <= self.dev.numel()
        assert 0 < self.values["WS_SLAM"] <= self.dev.numel() and 0 < self.values["WS_RANGES"] <= self.dev.numel()

    def call(self, entry, over):
        assert not set(over) - {k for k, _ in ENTRIES[entry]} - {"ctx", "failed_hip_call_first"}, (entry, over)
        args = [over.get(k, v) for k, v in ENTRIES[entry]]
        args = [self.values[a] if isinstance(a, str) else a for a in args]
        first = FIRST.get(entry, "ctx")
        if first:
            args.insert(0, over.get("ctx", self.g._h if first == "ctx" else self.group))
        if over.get("failed_hip_call_first"):  # (the library's own HIP runtime, on this thread)
            assert self.raw.hipSetDevice(1 << 20) != 0
        rc = getattr(self.raw if entry in MOVED or entry in MATCHER else self.lib, entry)(*args)
        if over.get("failed_hip_call_first"):
            self.raw.hipGetLastError()  # (nothing of it is left for the next launch check of this thread)
        return {"code": int(rc), "text": self.lib.hsm_last_error().decode() if rc != 0 else ""}

    def run(self, case_list):
        torch = self.torch
        got = {name: self.call(entry, over) for name, entry, over, capture in case_list if not capture}
        # the capture method of tests/test_gpu_update_scans_device.py: a graph of two trivial launches around the refused calls
        x = torch.zeros(8, device="cuda:0")
        self.stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=self.stream):
            x.add_(1.0)
            for name, entry, over, capture in case_list:
                if capture:
                    got[name] = self.call(entry, over)
            x.add_(1.0)
        torch.cuda.synchronize()
        return got

    def close(self):
        self.lib.hsm_group_destroy(self.group)
        self.g.synchronize()
        self.g.close()
