"""HIPBatch.select / selected / selectInfo (the N-API addon's batchSelect / batchSelected / batchSelectInfo): one golden fixture,
two streams of it, a few frames selected -- through decode(), decodeAsync() and enqueue(), and through HIPBatchRouter -- the
selected pictures' planes against the fixture's.  Needs an MI355X and node."""
import json
import os
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT
from jsmpeg_amd import build, synth

NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


def test_selected_frames_through_the_node_host(hip_lib):
    build.build_addon()
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "frames_cfg1_720p.json")))
    es, _ = synth.generate_config(fx["config"], n_frames=fx["n_frames"], **fx["overrides"])
    n = fx["n_frames"]                                   # 26 pictures, GOP 12: chains 0-11, 12-23, 24-25
    frames = [25, 3, 14]
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "s.m1v")
        es.tofile(path)
        r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "hip_batch_select.js"), path, str(fx["info"]["width"]),
                            str(fx["info"]["height"]), str(n), ",".join(map(str, frames))], capture_output=True, text=True, timeout=300)
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["ok"], res.get("error", "") + r.stderr[-2000:]
    assert res["whole"] == 2 * n and res["malformed"] == "TypeError" and res["outOfRange"] == "refused"
    # requests: (0, 25), (1, 3), (0, 14), (1, 100000); stream 1's pictures come behind stream 0's
    want_sel = [25, n + 3, 14, None]
    want_dec = [12, 13, 14, 24, 25] + [n + k for k in range(4)]
    for mode in ("decode", "decodeAsync", "enqueue"):
        m = res["modes"][mode]
        assert m["pictures"] == 2 * n and m["selected"] == want_sel, (mode, m)
        assert m["md5"] == [fx["frame_md5"][25], fx["frame_md5"][3], fx["frame_md5"][14], None], mode
        assert m["decoded"] == want_dec, (mode, m["decoded"])
        assert m["info"] == dict(selected=3, needed=len(want_dec), widenedStreams=0, redone=0), (mode, m["info"])
        assert [(f["stream"], f["index"], f["picture"]) for f in m["handed"]] == [(0, 14, 14), (0, 25, 25), (1, 3, n + 3)], mode
        assert [f["md5"] for f in m["handed"]] == [fx["frame_md5"][14], fx["frame_md5"][25], fx["frame_md5"][3]], mode
    assert res["inFlight"] == "refused"
    assert res["cleared"] == dict(pictures=2 * n, selected=[], decoded=2 * n)
    assert res["routerFrames"] == 2
    assert [(f["stream"], f["index"], f["md5"]) for f in res["router"]["handed"]] == [(0, 14, fx["frame_md5"][14]), (1, 25, fx["frame_md5"][25])]
    size = "%dx%d" % (fx["info"]["width"], fx["info"]["height"])
    assert res["router"]["selected"] == [dict(size=size, picture=n + 25), dict(size=size, picture=14)]
    assert res["router"]["info"] == {size: dict(selected=2, needed=5, widenedStreams=0, redone=0)}
