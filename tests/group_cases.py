"""The device group (hsm_group_*) across call sequences: the scene, the shard tables and the sequences of
hsm_group_match_batch_device calls that tests/test_gpu_group_sequences.py runs on ONE group each, from creation to close.  Every
sequence is named for the state transition of csrc/group.hip it is there for: a gathered row count that changes (the exchanges
are remade, the result blocks grow), a covariance array that comes and goes (the covariance exchange is made late, and goes
when only the pose exchange is remade), a root that moves, a first call whose root shard is empty, one shared scan in place of
CSR shards, a gather mode that changes, scans without beams.  tests/test_group_cases.py holds each sequence to its name.

Plain numpy, no GPU.  A call never gathers more than MAX_ROWS scans, a sequence has at most MAX_CALLS calls, a group REPLICAS
replicas."""
from typing import NamedTuple, Optional

import numpy as np

N_BEAMS, MAP_SIZE, LEVELS, RES = 360, 256, 3, 0.1
N_BUILD, N_QUERY, ROOM, SEED = 30, 48, (20.0, 15.0), 6113
REPLICAS, MAX_ROWS, MAX_CALLS = 3, 64, 8
DIRECT, PEER, RCCL = "direct", "peer", "rccl"

# the SLAM side: a rectangular map whose world origin is off its centre
SLAM_SX, SLAM_SY, SLAM_LEVELS, SLAM_START, SLAM_SEED = 320, 192, 4, (0.3, 0.6), 911
SLAM_FIRST, SLAM_DEVICE, SLAM_LAST = 10, 4, 5  # process_scan steps, scans of the device-resident writer, process_scan steps
SLAM_STEPS = SLAM_FIRST + 2 + SLAM_DEVICE + SLAM_LAST + 1  # (+ the step without an update, the empty scan's, one pose for the last hint)


class Call(NamedTuple):
    counts: tuple            # scans per replica
    root: int
    want_cov: bool
    mode: Optional[str] = None   # the gather mode set in front of this call (None: the sequence's, or what the last call left)


def _calls(*items):
    return [Call(*it) for it in items]


# form: "csr" ragged CSR shards; "shared" d_scan_offsets NULL, every row a pose hypothesis of ONE scan; "holes" CSR shards some of
# whose scans have no beams (HOLES: per call and replica, the rows of the shard that are empty)
SEQUENCES = {
    "totals": dict(form="csr", calls=_calls(((5, 5, 6), 2, True), ((16, 16, 16), 2, True), ((1, 0, 0), 2, True), ((0, 0, 0), 2, True),
                                            ((5, 5, 6), 2, True), ((21, 21, 22), 2, True))),
    "cov toggles": dict(form="csr", calls=_calls(((5, 5, 6), 2, True), ((5, 5, 6), 2, False), ((5, 5, 6), 2, True), ((7, 7, 7), 2, False),
                                                 ((7, 7, 7), 2, True), ((5, 5, 6), 2, True))),
    "root moves": dict(form="csr", calls=_calls(((5, 5, 6), 2, True), ((5, 5, 6), 0, True), ((5, 5, 6), 1, True), ((5, 5, 6), 2, True),
                                                ((6, 5, 5), 1, True), ((6, 5, 5), 0, True))),
    "empty first": dict(form="csr", calls=_calls(((0, 4, 0), 0, True), ((4, 0, 0), 2, True), ((0, 0, 4), 2, True))),
    "shared scan": dict(form="shared", calls=_calls(((7, 0, 9), 2, True), ((16, 0, 0), 2, True), ((5, 5, 6), 2, True))),
    "mode switches": dict(form="csr", calls=_calls(((5, 5, 6), 2, True, DIRECT), ((16, 16, 16), 2, True, PEER), ((16, 16, 16), 2, True, DIRECT),
                                                   ((5, 5, 6), 2, True, DIRECT), ((5, 5, 6), 2, True, PEER))),
    "empty scans": dict(form="holes", calls=_calls(((5, 5, 6), 1, True), ((5, 5, 6), 2, True))),
}
# shard 0: its first scan, shard 1: every scan, shard 2: its last scan; then first and last the other way round
HOLES = {"empty scans": [((0,), (0, 1, 2, 3, 4), (5,)), ((4,), (0, 1, 2, 3, 4), (0,))]}

# which sequences a gather mode runs: RCCL needs distinct devices (one replica per device the machine has), and gets the two
# sequences whose transitions it shares with the others -- the mode switches are between direct and peer
SEQUENCES_OF = {DIRECT: list(SEQUENCES), PEER: list(SEQUENCES), RCCL: ["totals", "cov toggles"]}

SHARED_SCAN = 5  # the query scan every row of a "shared" call is a hypothesis of
_WRAP_STEP = np.float32([0.02, -0.02, 0.01])  # a query scan that a call uses twice starts from another estimate the second time


def make_scene():
    from hector_slam_amd import synth
    return synth.make_scene(n_beams=N_BEAMS, map_size=MAP_SIZE, levels=LEVELS, resolution=RES, n_build=N_BUILD, n_query=N_QUERY, room=ROOM,
                            seed=SEED)


def first_rows(counts):
    """row of the gathered arrays at which each replica's shard starts, and the total behind them"""
    return np.concatenate([[0], np.cumsum(counts)]).astype(int)


def reshard(call, world):
    """the call for a group of `world` replicas: as it stands for REPLICAS; else the same total in the library's contiguous
    shards (the first total % world hold one scan more) and the root kept inside the group"""
    if world == REPLICAS:
        return call
    total = sum(call.counts)
    counts = tuple(total // world + (1 if r < total % world else 0) for r in range(world))
    return call._replace(counts=counts, root=min(call.root, world - 1))


def call_rows(name, k):
    """indices into a table of N_QUERY entries, one per gathered row of call k of the sequence, and how often the table has
    wrapped by then.  Every call of a sequence starts elsewhere in the table: a row that kept an earlier call's value differs
    from the value this call expects there"""
    total = sum(SEQUENCES[name]["calls"][k].counts)
    at = (5 * sorted(SEQUENCES).index(name) + 11 * k) % N_QUERY + np.arange(total)
    return at % N_QUERY, at // N_QUERY


def hypotheses(scene, n=N_QUERY):
    """start estimates around the shared scan's own"""
    d = np.random.default_rng(SEED + 7).uniform(-0.05, 0.05, (n, 3)).astype(np.float32) * np.float32([1, 1, 0.2])
    return scene.query_init[SHARED_SCAN] + d


def call_batch(scene, name, k):
    """(start estimates [total, 3], scans: a list of [n_i, 2] arrays in row order -- or, form "shared", the one scan) of call k"""
    seq = SEQUENCES[name]
    idx, wrap = call_rows(name, k)
    step = wrap[:, None].astype(np.float32) * _WRAP_STEP
    if seq["form"] == "shared":
        return np.ascontiguousarray(hypotheses(scene)[idx] + step, np.float32), scene.query_scans[SHARED_SCAN]
    init = np.ascontiguousarray(scene.query_init[idx] + step, np.float32)
    scans = [scene.query_scans[i] for i in idx]
    if seq["form"] == "holes":
        first = first_rows(seq["calls"][k].counts)
        for r, rows in enumerate(HOLES[name][k]):
            for j in rows:
                scans[first[r] + j] = np.zeros((0, 2), np.float32)
    return init, scans


def slam_scene():
    """(world, ground-truth poses, scans) of a loop in a room on the rectangular map"""
    import rect_cases
    return rect_cases.scene(SLAM_SX, SLAM_SY, SLAM_STEPS, N_BEAMS, SLAM_SEED, res=RES)
