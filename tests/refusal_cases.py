"""The refusals of the host runtime's scan-log, update and raw-scan entries, as a list of named cases: an entry of the C ABI plus
arguments that make it refuse before anything is queued.  tests/tools/record_host_refusals.py ran them on the commit before the
entries were rewritten onto argument bundles and wrote tests/golden/host_refusals.json (status code and the full hsm_last_error()
text of every case); tests/test_gpu_host_refusals.py replays them against the library under test and compares both exactly -- which
check wins where two apply, and the entry name in every text, are what such a rewrite can change silently.

Arguments are symbolic so that no address reaches the golden file: "D" a device buffer, "D+4" the same at an address 4 mod 8,
"D+1" at an odd one, "H" a host array, "S" the test's stream, None a null pointer.  No pointer is ever dereferenced: every case
refuses first.  Cases with capture=True run while "S" is being captured into a graph.
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
    assert len({c[0] for c in out}) == len(out)
    return out


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
        self.values = {
            "D": self.dev.data_ptr(), "D+4": self.dev.data_ptr() + 4, "D+1": self.dev.data_ptr() + 1, "H": self.host.ctypes.data,
            "H_DECREASING": self.decreasing.ctypes.data, "H_NEGATIVE": self.negative.ctypes.data, "S": self.stream.cuda_stream,
            "WS_RANGES": int(self.lib.hsm_match_batch_ranges_workspace(COUNT, N)),
            "WS_SLAM": int(self.lib.hsm_slam_ranges_tf_workspace(COUNT, N)),
        }
        self.values["WS_RANGES-1"] = self.values["WS_RANGES"] - 1
        self.values["WS_SLAM-1"] = self.values["WS_SLAM"] - 1
        assert 0 < self.values["WS_SLAM"] <= self.dev.numel() and 0 < self.values["WS_RANGES"] <= self.dev.numel()

    def call(self, entry, over):
        assert not set(over) - {k for k, _ in ENTRIES[entry]}, (entry, over)
        args = [over.get(k, v) for k, v in ENTRIES[entry]]
        args = [self.values[a] if isinstance(a, str) else a for a in args]
        rc = getattr(self.lib, entry)(self.g._h, *args)
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
        self.g.synchronize()
        self.g.close()
