"""jsmpeg_hip_batch_select: a pass over selected frames only -- the closure over forward references worked out on the device
(csrc/select_plan.h, kernels.hip k_select).  The golden fixtures and the oracle through both decode plans and enqueue, frames
nobody needed left unwritten, the widening of streams whose chain-start pictures leave macroblocks unwritten, tensors, the
refusals and the clearing.  The tests assert WORK DONE (counters), never times.  Needs an MI355X."""
import ctypes
import glob
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import ROOT
from jsmpeg_amd import batch as jb
from jsmpeg_amd import cabi, hashing, synth

pytestmark = pytest.mark.gpu

FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "frames_*.json"))) + \
           sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "enc1080", "frames_enc1080_*.json")))
MODES = ("levels", "auto", "enqueue")
PATTERN = 0xA5


def fixture_es(path):
    fx = json.load(open(path))
    if "enc1080" in os.path.basename(path):
        es = np.fromfile(os.path.join(os.path.dirname(path), fx["case"] + ".m1v"), dtype=np.uint8)
    else:
        es, _ = synth.generate_config(fx["config"], n_frames=fx["n_frames"], **fx["overrides"])
    assert hashlib.md5(es.tobytes()).hexdigest() == fx["es_md5"]
    fx.setdefault("info", dict(width=1920, height=1080))        # (the enc1080 GOPs' fixtures do not carry the size)
    return fx, es


def md5_planes(planes):
    h = hashlib.md5()
    for p in planes:
        h.update(p.tobytes())
    return h.hexdigest()


def oracle_hashes(libs, es):
    frames, _, _ = cabi.decode_stream(libs["oracle"], es, keep="planes")
    return [hashing.frame_hash(*f) for f in frames]


def run_pass(b, mode):
    if mode == "enqueue":
        b.set_reconstruct("auto")
        assert b.enqueue() == 0
        b.sync()
    else:
        b.set_reconstruct(mode)
        b.decode()


def fill_pool(b, n_pictures):
    L = b.L
    L.jsmpeg_hip_device_fill.restype = ctypes.c_int
    L.jsmpeg_hip_device_fill.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64]
    L.jsmpeg_hip_device_synchronize.restype = ctypes.c_int
    b.sync()
    assert L.jsmpeg_hip_device_fill(b.frame_pool_ptr, PATTERN, b.frame_stride * n_pictures) == 0
    assert L.jsmpeg_hip_device_synchronize() == 0


def pattern_hash(b):
    return hashing.frame_hash(np.full(b.luma_bytes + 2 * b.chroma_bytes, PATTERN, np.uint8))


class Whole:
    """the whole decode's picture table, and the brute-force closure of a selection over it"""

    def __init__(self, b):
        self.info = b.pictures()
        self.uncovered = b.uncovered()
        self.frames = {}
        for p, i in enumerate(self.info):
            if i.decoded:
                self.frames.setdefault(i.stream, []).append(p)

    def picture(self, stream, frame):
        f = self.frames.get(stream, [])
        return f[frame] if frame < len(f) else None

    def closure(self, reqs):
        needed = set()
        for s, f in reqs:
            p = self.picture(s, f)
            while p is not None and p >= 0 and p not in needed:
                needed.add(p)
                p = self.info[p].forward
        return needed

    def chains(self, stream):
        """the stream's decoded pictures cut at every one without a forward reference: lists of FRAME numbers"""
        out = []
        for f, p in enumerate(self.frames.get(stream, [])):
            if self.info[p].forward < 0 or not out:
                out.append([])
            out[-1].append(f)
        return out

    def inexact(self, needed):
        """streams in which a needed picture with unwritten macroblocks shows, in the thinned pass, another frame than the whole
        decode's decoded picture before last: the ones the engine has to widen"""
        bad = set()
        for s, fr in self.frames.items():
            thin = [p for p in fr if p in needed]
            for k, p in enumerate(thin):
                i = fr.index(p)
                whole = fr[i - 2] if i >= 2 else -1
                used = thin[k - 2] if k >= 2 else -1
                if self.uncovered[p] and whole != used:
                    bad.add(s)
        return bad

    def prefix(self, needed, streams):
        out = set(needed)
        for s in streams:
            fr = self.frames[s]
            last = max(i for i, p in enumerate(fr) if p in needed)
            out |= set(fr[:last + 1])
        return out


def check_selected_pass(b, w, reqs, want_md5=None, want_hash=None, tag=""):
    """everything a selected pass promises, against the whole decode's table `w`; returns (needed set, select_info)"""
    info = b.pictures()
    assert b.picture_count == len(w.info)
    assert [(i.stream, i.es_offset, i.type) for i in info] == [(i.stream, i.es_offset, i.type) for i in w.info], tag
    sel = b.selected()
    assert sel == [w.picture(s, f) for s, f in reqs], tag
    needed = w.closure(reqs)
    si = b.select_info()
    bad = w.inexact(needed)
    print("select", tag, "requests", len(reqs), "needed", len(needed), "of", sum(len(f) for f in w.frames.values()), "info", si,
          "streams to widen", sorted(bad))
    # (the selection was set right before this pass: nothing widened is left over from an earlier one)
    assert si["widened_streams"] == len(bad) and si["redone"] == (1 if bad else 0), tag
    needed = w.prefix(needed, bad)
    assert {p for p, i in enumerate(info) if i.decoded} == needed, tag
    assert si["selected"] == len({p for p in sel if p is not None}) and si["needed"] == len(needed), tag
    c = b.counters()
    assert c["decoded"] == len(needed) and c["slices"] == sum(w.info[p].n_slices for p in needed), (tag, c)
    assert c["pictures"] == len(w.info)
    for (s, f), p in zip(reqs, sel):
        if p is None:
            continue
        if want_md5 is not None:
            assert md5_planes(b.read_frame(p)) == want_md5[s][f], (tag, s, f, p)
    hashes = [int(h) for h in b.frame_hashes()]
    if want_hash is not None:
        for p in needed:
            assert hashes[p] == want_hash[p], (tag, p)
    return needed, si, hashes


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[7:-5] for p in FIXTURES])
def test_golden_fixture_selected(path, hip_lib):
    """every fixture, three selections (the last frame, frame 0, two frames in different GOPs where the stream has two), each
    through decode level by level, decode as created and enqueue: the selected pictures are the golden ones, the table is the
    whole decode's but for `decoded`, which is 1 exactly on the closure (a widened stream's: on the prefix), the counters are
    the closure's sums, and every frame that was not needed still holds the pattern the pool was filled with"""
    fx, es = fixture_es(path)
    n = len(fx.get("abi_frame_md5", fx["frame_md5"]))
    with jb.Batch(fx["info"]["width"], fx["info"]["height"], 1, n + 4, len(es) + 8192) as b:
        b.upload([es])
        assert b.decode() == n
        w = Whole(b)
        n_frames = len(w.frames[0])
        assert n_frames == fx["n_frames"]
        selections = [[(0, n_frames - 1)], [(0, 0)]]
        ch = w.chains(0)
        if len(ch) >= 2:
            selections.append([(0, ch[-1][len(ch[-1]) // 2]), (0, ch[0][-1])])
        blank = pattern_hash(b)
        for reqs in selections:
            for mode in MODES:
                b.select(reqs)                       # (again for every mode: a widening stays with the selection otherwise)
                fill_pool(b, n)
                run_pass(b, mode)
                tag = "%s %s %s" % (fx["case"], reqs, mode)
                needed, si, hashes = check_selected_pass(b, w, reqs, want_md5=[fx["frame_md5"]], tag=tag)
                for p in range(n):
                    if p not in needed:
                        assert hashes[p] == blank, (tag, p)
                if mode == "enqueue" and not si["redone"]:
                    assert b.timings()["host_ms"] == 0.0
        b.select(None)
        b.decode()
        assert [(i.decoded, i.n_slices) for i in b.pictures()] == [(i.decoded, i.n_slices) for i in w.info]


def sixteen_streams(libs):
    streams, want = [], []
    for s in range(16):
        es, _ = synth.generate_config("cfg1_720p", n_frames=24, stream=s % 4, width=640, height=368, gop=(6 if s % 2 else 12))
        streams.append(es)
        want += oracle_hashes(libs, es)
    return streams, want


def test_random_selections_against_the_oracle(hip_lib, libs):
    """sixteen streams of 24 pictures (GOP 6 and 12): 20 seeded random selections of 1 .. 6 frames per stream, some streams with
    none, through both decode plans and enqueue; the selected (and every needed) picture's device hash is the oracle's"""
    streams, want = sixteen_streams(libs)
    rng = np.random.default_rng(1016)
    os.environ["JSMPEG_HIP_RECON_ORDER"] = "2"          # (read when a batch is created: the ordered launch where it can be taken)
    try:
        b = jb.Batch(640, 368, 16, len(want) + 8, sum(len(s) for s in streams) + 8192)
    finally:
        os.environ.pop("JSMPEG_HIP_RECON_ORDER", None)
    with b:
        b.upload(streams)
        b.decode()
        w = Whole(b)
        assert [int(h) for h in b.frame_hashes()] == want
        ordered = 0
        for k in range(20):
            reqs = []
            for s in range(16):
                if rng.random() < 0.2:
                    continue
                reqs += [(s, int(f)) for f in rng.integers(0, 24, int(rng.integers(1, 7)))]
            reqs = [reqs[i] for i in rng.permutation(len(reqs))]
            b.select(reqs)
            for mode in MODES:
                run_pass(b, mode)
                needed, si, _ = check_selected_pass(b, w, reqs, want_hash=want, tag="random %d %s" % (k, mode))
                assert si["widened_streams"] == 0
                info = b.recon_info()
                if info["launches"] == 1 and info["group"]:
                    ordered += 1
                    assert info["status"] == 0, info
                if mode == "levels":
                    assert info["group"] == 0
                if mode == "enqueue":
                    assert b.timings()["host_ms"] == 0.0
                    assert info["status"] in (0, 8), info
        print("passes that took the ordered launch:", ordered)


def widening_inputs():
    out = []
    for path in FIXTURES:
        name = os.path.basename(path)
        if name.startswith("frames_uncovered_") or name.startswith("frames_syntax_quirks_"):
            fx, es = fixture_es(path)
            out.append((fx["case"], es, fx["info"]["width"], fx["info"]["height"]))
    es, _ = synth.generate_config("cfg1_720p", n_frames=36, stream=11, width=352, height=288, gop=3, mv_jitter=1, f_code_max=1,
                                  coded_permille=60, ac_max=1)
    out.append(("synth_mv_jitter_352x288", es, 352, 288))
    return out


def test_widening_is_exact(hip_lib, libs):
    """streams whose chain-start pictures leave macroblocks unwritten: a selection of such a picture alone has its decoded picture
    before last -- in the GOP in front -- outside the closure; the stream is widened, the pass done over, and every selected picture
    is bit for bit the oracle's.  A selection in the same streams that needs no widening reports none."""
    found = 0
    for case, es, width, height in widening_inputs():
        want = oracle_hashes(libs, es)
        with jb.Batch(width, height, 1, len(want) + 40, len(es) + 8192) as b:
            b.upload([es])
            b.decode()
            w = Whole(b)
            assert [int(h) for h, i in zip(b.frame_hashes(), w.info) if i.decoded] == want
            want_by_picture = {p: want[f] for f, p in enumerate(w.frames[0])}
            fr = w.frames[0]
            # a chain's first or second picture with unwritten macroblocks and a decoded picture two places in front of it
            cand = []
            for chain in w.chains(0)[1:]:
                for f in chain[:2]:
                    if w.uncovered[fr[f]] and f >= 2 and fr[f - 2] not in w.closure([(0, f)]):
                        cand.append(f)
            print("widening", case, "uncovered frames", [f for f, p in enumerate(fr) if w.uncovered[p]], "candidates", cand)
            for f in cand[:3]:
                found += 1
                reqs = [(0, f)]
                assert w.inexact(w.closure(reqs)) == {0}            # the precondition, from the whole decode alone
                for mode in MODES:
                    b.select(reqs)
                    run_pass(b, mode)
                    si = b.select_info()
                    assert si["widened_streams"] >= 1 and si["redone"] == 1, (case, f, mode, si)
                    p = b.selected()[0]
                    assert p == fr[f]
                    hashes = [int(h) for h in b.frame_hashes()]
                    assert hashes[p] == want_by_picture[p], (case, f, mode)
                    # what the widened pass decoded: the prefix, all of it the oracle's
                    dec = [q for q, i in enumerate(b.pictures()) if i.decoded]
                    assert dec == fr[:f + 1]
                    assert [hashes[q] for q in dec] == want[:f + 1]
                    # the widening stays: the same pass again is not done over
                    run_pass(b, mode)
                    si = b.select_info()
                    assert si["widened_streams"] >= 1 and si["redone"] == 0
                    assert int(b.frame_hashes()[p]) == want_by_picture[p]
            # no widening: frame 0 (nothing in front of it), and a whole chain's last frame together with the chains before it
            for reqs in ([(0, 0)], [(0, c[-1]) for c in w.chains(0)[:2]]):
                if w.inexact(w.closure(reqs)):
                    continue
                for mode in MODES:
                    b.select(reqs)
                    run_pass(b, mode)
                    si = b.select_info()
                    assert si["widened_streams"] == 0 and si["redone"] == 0, (case, reqs, mode, si)
                    for (s, f), p in zip(reqs, b.selected()):
                        assert int(b.frame_hashes()[p]) == want_by_picture[p]
    assert found >= 1, "no input has a chain-start picture with unwritten macroblocks and a decoded picture two places in front"


def test_tensor_of_selected_pictures(hip_lib, libs):
    torch = pytest.importorskip("torch")
    streams, _ = sixteen_streams(libs)
    reqs = [(s, (5 * s + 3) % 24) for s in range(16)] + [(3, 23), (3, 23), (7, 0)]
    with jb.Batch(640, 368, 16, 16 * 24 + 8, sum(len(s) for s in streams) + 8192) as b:
        b.upload(streams)
        b.decode()
        w = Whole(b)
        pics = [w.picture(s, f) for s, f in reqs]
        want = b.tensor(pictures=pics, size=(224, 224), dtype="float16").clone()
        b.select(reqs)
        for mode in MODES:
            run_pass(b, mode)
            assert b.selected() == pics
            got = b.tensor(pictures=b.selected(), size=(224, 224), dtype="float16")
            assert torch.equal(got, want), mode
        # a picture that was not needed is refused as every picture that was not decoded is
        spare = next(p for p, i in enumerate(b.pictures()) if not i.decoded)
        with pytest.raises(RuntimeError, match="was not decoded"):
            b.tensor(pictures=[spare], size=(224, 224), dtype="float16")


def test_refusals_and_clearing(hip_lib, libs):
    es, _ = synth.generate_config("cfg1_720p", n_frames=12, stream=5, width=176, height=144, gop=4)
    want = oracle_hashes(libs, es)
    with jb.Batch(176, 144, 8, 8 * 12 + 8, 8 * (len(es) + 64) + 8192) as b:
        b.upload([es] * 8)
        b.decode()
        whole = [(i.decoded, i.n_slices) for i in b.pictures()]
        # a selection and links / seeds: the pass is refused, in either order, and names both
        for first in ("select", "links", "seed"):
            b.upload([es] * 8)
            if first == "select":
                b.select([(0, 3)])
                b.link_streams([-1] * 8)
            elif first == "links":
                b.link_streams([-1] * 8)
                b.select([(0, 3)])
            else:
                b.seed_stream(1, None, None)
                b.select([(0, 3)])
            for call in (b.decode, b.enqueue):
                with pytest.raises(RuntimeError, match="selection.*linked or seeded"):
                    call()
        b.upload([es] * 8)
        with pytest.raises(RuntimeError, match="stream 8 of 8"):
            b.select([(0, 1), (8, 0)])
        b.select([(2, 5), (2, 99)])
        assert b.enqueue() == 0
        with pytest.raises(RuntimeError, match="in flight"):
            b.select([(0, 0)])
        b.sync()
        assert b.selected() == [2 * 12 + 5, None]
        assert b.select_info() == dict(selected=1, needed=2, widened_streams=0, redone=0)     # frames 4 and 5 of stream 2
        assert [p for p, i in enumerate(b.pictures()) if i.decoded] == [2 * 12 + 4, 2 * 12 + 5]
        with pytest.raises(RuntimeError, match="was not decoded"):
            b.tensor(pictures=[0], size=(32, 32))
        assert int(b.frame_hashes()[2 * 12 + 5]) == want[5]
        # select(None) clears; so does the next upload
        b.select(None)
        b.decode()
        assert [(i.decoded, i.n_slices) for i in b.pictures()] == whole and [int(h) for h in b.frame_hashes()] == want * 8
        assert b.selected() == []
        b.select([(1, 1)])
        b.upload([es] * 8)
        assert b.enqueue() == 0
        b.sync()
        assert [(i.decoded, i.n_slices) for i in b.pictures()] == whole and [int(h) for h in b.frame_hashes()] == want * 8
        assert b.select_info() == dict(selected=0, needed=0, widened_streams=0, redone=0)
