"""A refused chain queues nothing, on the MI355X.

hsm_match_score_batch_device, hsm_match_cov_batch_device and hsm_relocalize_device queue a match, a scoring step at the matched
poses and the winners under one lock, and check every argument before the first launch.  Each is called here with an argument that
only the LAST step of its chain objects to (one group of 5 in a batch of 4; for the relocalisation a null best_index): the call
returns HSM_ERR_INVALID and, once the stream has drained, every output buffer still holds the bit pattern it was filled with --
the poses and covariances included, which the match would have written.  The same call with the argument mended then gives, bit
for bit, what the chain's steps give as separate calls.

Streams: the device entries take the caller's stream, and the context's own is not handed out, so each device entry runs on the
null stream and on a stream of the test's; the chain on the context's own stream is what the host entries hsm_match_score_batch
and hsm_relocalize run, and they are held to the same two properties (hsm_match_cov_batch_device has no host form).

Map: 2 levels of 64 x 64 cells built from two scans of a 4 m x 3 m room; 4 start poses against one shared scan of 32 beams.
"""
import ctypes as C

import numpy as np
import pytest

from support import capi, new_context, single_update  # noqa: F401

pytestmark = pytest.mark.gpu

HSM_ERR_INVALID = -1
SENT = 0x5A5A5A5A  # every word of every output buffer before a call
B, BEAMS, K = 4, 32, 2
STEP, HALF, SEARCH_LEVEL = (0.1, 0.1, 0.05), (1, 1, 0), 1
W = 9


def room_scan(pose, beams):
    """the walls of a 4 m x 3 m room around the world's origin as seen from `pose`: end points in the sensor frame, level-0 cells"""
    x, y, th = pose
    a = th + np.linspace(-np.pi, np.pi, beams, endpoint=False)
    dx, dy = np.cos(a), np.sin(a)
    with np.errstate(divide="ignore"):
        tx = np.where(dx > 0, (2.0 - x) / dx, (-2.0 - x) / dx)
        ty = np.where(dy > 0, (1.5 - y) / dy, (-1.5 - y) / dy)
    r = np.minimum(np.where(np.isfinite(tx), tx, np.inf), np.where(np.isfinite(ty), ty, np.inf))
    b = a - th
    return np.ascontiguousarray(np.stack([r * np.cos(b), r * np.sin(b)], 1) * 10.0, np.float32)


@pytest.fixture(scope="module")
def world(capi):  # noqa: F811
    import torch
    g = new_context(capi, 0.1, 64, 64, 2)
    for pose in ((0.0, 0.0, 0.0), (0.1, 0.05, 0.05)):
        single_update(capi, g, np.float32(pose), room_scan(pose, 181))
    g.synchronize()
    starts = np.float32([[0.05, 0.0, 0.0], [0.0, 0.05, 0.02], [-0.05, 0.05, -0.02], [0.02, -0.03, 0.01]])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")  # noqa: E731
    yield dict(g=g, lib=capi.load_library(), starts=starts, scan=room_scan((0.0, 0.0, 0.0), BEAMS), d_starts=d(starts),
               d_scan=d(room_scan((0.0, 0.0, 0.0), BEAMS)), d_center=d(np.float32([0.03, -0.02, 0.01])))
    g.close()


def buffers(**words):
    """device buffers of int32 words, every word SENT"""
    import torch
    bufs = {k: torch.full((n,), SENT, dtype=torch.int32, device="cuda:0") for k, n in words.items()}
    torch.cuda.synchronize()  # (filled on torch's stream, handed to others)
    return bufs


def untouched(bufs):
    return all(bool((b == SENT).all()) for b in bufs.values())


def same_words(got, want, keys):
    for k in keys:
        assert np.array_equal(got[k].cpu().numpy(), want[k].cpu().numpy()), k


def streams():
    import torch
    return [("null stream", None, None), ("own stream", *(lambda s: (s, s.cuda_stream))(torch.cuda.Stream()))]


def drain(stream):
    import torch
    torch.cuda.synchronize()


CHAIN_OUT = dict(pose=B * 3, cov=B * 9, idx=1, score=1, bpose=3)


@pytest.mark.parametrize("entry", ["hsm_match_score_batch_device", "hsm_match_cov_batch_device"])
def test_refused_match_chain_queues_nothing_and_mended_equals_its_steps(world, entry):
    g, lib = world["g"], world["lib"]
    cov = entry == "hsm_match_cov_batch_device"
    mid = dict(cw=B * 9, cm=B * 9, l7=B * 7, lh=B) if cov else dict(lh=B, res=B)
    p = lambda t: t.data_ptr()  # noqa: E731
    for name, _, s in streams():
        o = buffers(**CHAIN_OUT, **mid)
        mid_args = (p(o["cw"]), p(o["cm"]), p(o["l7"]), p(o["lh"])) if cov else (p(o["lh"]), p(o["res"]))

        def chain(group_size):
            return getattr(lib, entry)(g._h, B, p(world["d_starts"]), p(world["d_scan"]), None, BEAMS, p(o["pose"]), p(o["cov"]), 0,
                                       *mid_args, 1, None, group_size, p(o["idx"]), p(o["score"]), p(o["bpose"]), s)
        assert chain(B + 1) == HSM_ERR_INVALID, name
        assert entry.encode() in lib.hsm_last_error()
        drain(s)
        assert untouched(o), f"{entry} on the {name}: a refused chain wrote an output"
        assert chain(B) == 0, lib.hsm_last_error()
        drain(s)
        # the steps as separate calls, into buffers of their own
        r = buffers(**CHAIN_OUT, **mid)
        g.match_batch_device(B, p(world["d_starts"]), p(world["d_scan"]), 0, BEAMS, p(r["pose"]), p(r["cov"]), s or 0)
        if cov:
            g.covariance_batch_device(0, B, p(r["pose"]), p(world["d_scan"]), 0, BEAMS, p(r["cw"]), p(r["cm"]), p(r["l7"]), p(r["lh"]), s or 0)
        else:
            g.score_batch_device(0, B, p(r["pose"]), p(world["d_scan"]), 0, BEAMS, p(r["lh"]), p(r["res"]), s or 0)
        g.select_best_device(1, 0, B, p(r["lh"]), p(r["pose"]), p(r["idx"]), p(r["score"]), p(r["bpose"]), s or 0)
        drain(s)
        assert not untouched({k: v for k, v in o.items() if k in ("pose", "lh", "idx")})
        same_words(o, r, list(o))
        assert 0 <= int(o["idx"].item()) < B


RELOC_OUT = dict(cpose=K * 3, ccov=K * 9, clh=K, bpose=3, bscore=1, bidx=1)


def relocalize_steps(world, s):
    """window score -> top K -> poses -> match -> score on level 0 -> winner as separate calls; -> buffers named as RELOC_OUT"""
    g = world["g"]
    p = lambda t: t.data_ptr()  # noqa: E731
    r = buffers(**RELOC_OUT, scores=W, kindex=K, kscore=K, kpose=K * 3, sel=1)
    ws = buffers(ws=(g.select_topk_workspace(W, K) + 3) // 4)["ws"]
    g.score_window_device(SEARCH_LEVEL, p(world["d_center"]), STEP, HALF, p(world["d_scan"]), BEAMS, p(r["scores"]), 0, s or 0)
    g.select_topk_device(W, p(r["scores"]), K, p(r["kindex"]), p(r["kscore"]), p(ws), ws.numel() * 4, s or 0)
    g.window_poses_device(p(world["d_center"]), STEP, HALF, p(r["kindex"]), K, p(r["kpose"]), s or 0)
    g.match_batch_device(K, p(r["kpose"]), p(world["d_scan"]), 0, BEAMS, p(r["cpose"]), p(r["ccov"]), s or 0)
    g.score_batch_device(0, K, p(r["cpose"]), p(world["d_scan"]), 0, BEAMS, p(r["clh"]), 0, s or 0)
    g.select_best_device(1, 0, K, p(r["clh"]), p(r["cpose"]), p(r["sel"]), p(r["bscore"]), p(r["bpose"]), s or 0)
    drain(s)
    sel = int(r["sel"].item())
    r["bidx"][0] = int(r["kindex"][sel].item()) if sel >= 0 else -1  # the window index of the winner's start
    return r


def test_refused_relocalisation_queues_nothing_and_mended_equals_its_steps(world):
    g, lib = world["g"], world["lib"]
    p = lambda t: t.data_ptr()  # noqa: E731
    st, hf = g._window(STEP, HALF)
    ws_bytes = g.relocalize_workspace(W, K)
    for name, _, s in streams():
        o = buffers(**RELOC_OUT, ws=(ws_bytes + 3) // 4 + 2)
        assert p(o["ws"]) % 8 == 0

        def chain(bidx):
            return lib.hsm_relocalize_device(g._h, SEARCH_LEVEL, p(world["d_center"]), st, hf, K, p(world["d_scan"]), BEAMS, p(o["ws"]),
                                             ws_bytes, p(o["cpose"]), p(o["ccov"]), p(o["clh"]), p(o["bpose"]), p(o["bscore"]), bidx, s)
        assert chain(None) == HSM_ERR_INVALID, name
        assert b"hsm_relocalize_device" in lib.hsm_last_error()
        drain(s)
        assert untouched(o), f"hsm_relocalize_device on the {name}: a refused chain wrote an output or its workspace"
        assert chain(p(o["bidx"])) == 0, lib.hsm_last_error()
        drain(s)
        r = relocalize_steps(world, s)
        same_words(o, r, list(RELOC_OUT))
        assert int(o["bidx"].item()) >= 0


def test_host_chains_on_the_contexts_stream_refuse_whole_and_equal_the_device_chain(world):
    """hsm_match_score_batch and hsm_relocalize: the same chains on the context's own stream"""
    g, lib = world["g"], world["lib"]
    h = {k: np.full(n, SENT, np.int32) for k, n in dict(**CHAIN_OUT, lh=B, res=B).items()}
    a = lambda k: h[k].ctypes.data  # noqa: E731
    starts, scan = world["starts"], world["scan"]

    def host_chain(group_size):
        return lib.hsm_match_score_batch(g._h, B, starts.ctypes.data, scan.ctypes.data, None, BEAMS, a("pose"), a("cov"), 0, a("lh"),
                                         a("res"), 1, None, group_size, a("idx"), a("score"), a("bpose"))
    assert host_chain(B + 1) == HSM_ERR_INVALID
    assert lib.hsm_last_error() == b"hsm_match_score_batch: bad argument"
    g.synchronize()
    assert all((v == SENT).all() for v in h.values())
    h["bpose"][:] = np.float32([0, 0, 0]).view(np.int32)  # (in/out: a group without a winner keeps it)
    assert host_chain(B) == 0, lib.hsm_last_error()
    p = lambda t: t.data_ptr()  # noqa: E731
    o = buffers(**CHAIN_OUT, lh=B, res=B)
    g.match_score_batch_device(B, p(world["d_starts"]), p(world["d_scan"]), 0, BEAMS, p(o["pose"]), p(o["cov"]), 0, p(o["lh"]),
                               p(o["res"]), 1, 0, B, p(o["idx"]), p(o["score"]), p(o["bpose"]), 0)
    drain(None)
    for k in h:
        assert np.array_equal(h[k], o[k].cpu().numpy()), k
    # the relocalisation
    r = {k: np.full(n, SENT, np.int32) for k, n in RELOC_OUT.items()}
    b = lambda k: r[k].ctypes.data  # noqa: E731
    st, hf = g._window(STEP, HALF)
    center = np.float32([0.03, -0.02, 0.01])

    def host_reloc(bidx):
        return lib.hsm_relocalize(g._h, SEARCH_LEVEL, center.ctypes.data, st, hf, K, scan.ctypes.data, BEAMS, b("cpose"), b("ccov"),
                                  b("clh"), b("bpose"), b("bscore"), bidx)
    assert host_reloc(None) == HSM_ERR_INVALID
    assert lib.hsm_last_error() == b"hsm_relocalize: bad argument"
    g.synchronize()
    assert all((v == SENT).all() for v in r.values())
    r["bpose"][:] = np.float32([0, 0, 0]).view(np.int32)
    assert host_reloc(C.c_void_p(b("bidx"))) == 0, lib.hsm_last_error()
    want = relocalize_steps(world, None)
    for k in RELOC_OUT:
        assert np.array_equal(r[k], want[k].cpu().numpy()), k
