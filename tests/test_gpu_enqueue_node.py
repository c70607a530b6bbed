"""HIPBatch.prototype.enqueue (the N-API addon's batchEnqueue / batchQuery / batchSync): two batches in flight from one Node
event loop with no thread of libuv's pool -- UV_THREADPOOL_SIZE=1 while a long crypto.pbkdf2 holds that thread, and every pass
of both batches finishes first, each picture against the oracle.  Needs an MI355X and node."""
import json
import os
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT
from jsmpeg_amd import build, cabi, hashing, synth

NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


def test_two_batches_enqueued_from_one_event_loop_take_no_pool_thread(hip_lib):
    build.build_addon()
    lib = build.build_oracle()
    sets = {"A": [synth.generate_config("cfg1_720p", n_frames=12, width=352, height=288, stream=s, gop=6)[0] for s in range(8)],
            "B": [synth.generate_config("cfg1_720p", n_frames=9, width=352, height=288, stream=10 + s, gop=4)[0] for s in range(12)]}
    want = {k: [["%016x" % hashing.frame_hash(*f) for f in cabi.decode_stream(lib, es, keep="planes")[0]] for es in v] for k, v in sets.items()}
    with tempfile.TemporaryDirectory() as td:
        dirs = {}
        for k, v in sets.items():
            dirs[k] = os.path.join(td, k)
            os.makedirs(dirs[k])
            for i, es in enumerate(v):
                es.tofile(os.path.join(dirs[k], "s%d.m1v" % i))
        hp = os.path.join(td, "hashes.json")
        json.dump(want, open(hp, "w"))
        env = dict(os.environ, UV_THREADPOOL_SIZE="1")
        r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "hip_batch_enqueue.js"), hp, "352", "288", dirs["A"], "8", dirs["B"], "12", "4"],
                           env=env, capture_output=True, text=True, timeout=300)
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["ok"], res.get("error", "") + r.stderr[-2000:]
    assert res["picturesA"] == [96] * 4 and res["picturesB"] == [108] * 4
    assert res["pbkdf2_before"] is False and res["order"][:2] in (["A", "B"], ["B", "A"]), res
    assert res["second"] == "refused"
