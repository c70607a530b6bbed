"""Part 7 on the GPU: decoded pictures as resized RGB tensors (Batch.tensor, Live.tensor, Live.latest_tensor -> k_tensor).
Source of truth: the planes are pinned to the golden frame md5s first; the expected tensor is then computed on the host
(numpy integer RGB, torch CPU resize and normalisation: tests/tensor_ref.py), never by another GPU path."""
import glob
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from jsmpeg_amd import batch as jb, live as jl, synth
from tensor_ref import DTYPES, IMAGENET_MEAN, IMAGENET_STD, check, planes, reference, rgb

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "frames_*.json")))


def load(name):
    path = os.path.join(GOLDEN, name if name.endswith(".json") else "frames_%s.json" % name)
    if not os.path.exists(path):
        path = os.path.join(GOLDEN, "enc1080", "frames_%s.json" % name)
    fx = json.load(open(path))
    if os.path.dirname(path).endswith("enc1080"):
        es = np.fromfile(os.path.join(os.path.dirname(path), fx["case"] + ".m1v"), dtype=np.uint8)
        fx.setdefault("info", {"width": 1920, "height": 1080})
    else:
        es, _ = synth.generate_config(fx["config"], n_frames=fx["n_frames"], **fx["overrides"])
    assert hashlib.md5(es.tobytes()).hexdigest() == fx["es_md5"]
    return fx, es


def md5_planes(y, cr, cb):
    h = hashlib.md5()
    for p in (y, cr, cb):
        h.update(p.tobytes())
    return h.hexdigest()


def decoded_batch(fx, es, n_streams=1, levels=False):
    """a batch of n_streams copies of the stream, decoded and synchronised; returns (batch, decoded picture indices)"""
    w, h = fx["info"]["width"], fx["info"]["height"]
    n_pics = len(fx.get("abi_frame_md5", fx["frame_md5"])) + 2
    b = jb.Batch(w, h, n_streams, n_pics * n_streams, (len(es) + 1024) * n_streams, device=0)
    if levels:
        b.set_reconstruct("levels")
    b.upload([es] * n_streams)
    b.decode()
    dec = [p for p, i in enumerate(b.pictures()) if i.decoded]
    assert len(dec) == fx["n_frames"] * n_streams
    return b, dec


def pinned_rgb(b, fx, p, k=None):
    """picture p's integer RGB from its planes, which first must be the golden ones (decoded picture k of its stream)"""
    y, cr, cb = b.read_frame(p)
    if k is not None:
        assert md5_planes(y, cr, cb) == fx["frame_md5"][k]
    return rgb(*planes(np.concatenate([y, cr, cb]), b.coded_width, b.coded_height), b.width, b.height)


def as_nchw(t, layout):
    return t.permute(0, 3, 1, 2) if layout == "nhwc" else t


# ---------------------------------------------------------------------------------------------------------- identity

@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[7:-5] for p in FIXTURES])
def test_identity_u8(path):
    fx, es = load(os.path.basename(path))
    b, dec = decoded_batch(fx, es)
    with b:
        pics = dec[:4]
        w, h = b.width, b.height
        want = [pinned_rgb(b, fx, p, k) for k, p in enumerate(pics)]
        nhwc = b.tensor(pics, dtype=torch.uint8, layout="nhwc").cpu().numpy()
        nchw_bgr = b.tensor(pics, dtype="uint8", order="bgr").cpu().numpy()
        for k, p in enumerate(pics):
            assert np.array_equal(nhwc[k].transpose(2, 0, 1), want[k]), "picture %d" % p
            assert np.array_equal(nchw_bgr[k][::-1], want[k]), "picture %d (NCHW, BGR)" % p
            if w % 2 == 0:
                rows = h if h % 2 == 0 else h - 1        # (odd heights: the reference's loop never writes the last row)
                assert np.array_equal(nhwc[k][:rows], b.read_rgba(p)[:rows, :, :3]), "picture %d differs from read_rgba" % p


# ------------------------------------------------------------------------------------------------------------ resize

RESIZE = {
    "aa_224": dict(size=(224, 224)),
    "plain_224": dict(size=(224, 224), antialias=False),
    "aa_320x180": dict(size=(180, 320)),
    "crop_resize": dict(size=(160, 96), crop=(101, 37, 333, 251)),
    "imagenet_224": dict(size=(224, 224), mean=IMAGENET_MEAN, std=IMAGENET_STD),
}


@pytest.mark.parametrize("fixture", ["cfg2_1080p", "cfg1_720p", "enc1080_0"])
def test_resize_every_dtype_and_layout(fixture):
    fx, es = load(fixture)
    b, dec = decoded_batch(fx, es)
    with b:
        pics = [dec[0], dec[len(dec) // 2]]
        src = [pinned_rgb(b, fx, p, dec.index(p)) for p in pics]
        for name, kw in RESIZE.items():
            crop = kw.get("crop")
            ref_kw = dict(size=kw["size"], crop=crop, antialias=kw.get("antialias", True))
            want = [reference(s, mean=kw.get("mean"), std=kw.get("std"), **ref_kw) for s in src]
            want_u8 = [reference(s, u8=True, **ref_kw) for s in src]
            for dname, dt in DTYPES.items():
                for layout in ("nchw", "nhwc"):
                    t = b.tensor(pics, dtype=dt, layout=layout, **kw)
                    assert t.device == torch.device("cuda", 0) and t.dtype == dt and t.is_contiguous()
                    t = as_nchw(t, layout).cpu()
                    for k in range(len(pics)):
                        check(t[k], want_u8[k] if dt == torch.uint8 else want[k], dt)


def test_upscale_2x():
    fx, es = load("coherent_pan_352x288")
    b, dec = decoded_batch(fx, es)
    with b:
        p = dec[5]
        src = pinned_rgb(b, fx, p, 5)
        for aa in (True, False):
            for dname, dt in DTYPES.items():
                for layout in ("nchw", "nhwc"):
                    t = as_nchw(b.tensor([p], size=(576, 704), dtype=dt, layout=layout, antialias=aa), layout).cpu()
                    check(t[0], reference(src, (576, 704), None, aa, u8=dt == torch.uint8), dt)


GEOMETRY = {
    "1080p_to_1x1": ("cfg2_1080p", dict(size=(1, 1))),
    "1080p_to_7x1": ("cfg2_1080p", dict(size=(7, 1))),            # 1920 -> 1: one lane, 1920 taps, chunks of 4 source rows
    "1080p_to_1x224": ("cfg2_1080p", dict(size=(1, 224))),
    "crop_up_to_4096_wide": ("cfg2_1080p", dict(size=(40, 4096), crop=(333, 101, 64, 17))),
    "352x288_up_to_4096x2048": ("coherent_pan_352x288", dict(size=(2048, 4096))),
}


@pytest.mark.parametrize("case", sorted(GEOMETRY))
def test_geometry_extremes(case):
    fixture, kw = GEOMETRY[case]
    fx, es = load(fixture)
    b, dec = decoded_batch(fx, es)
    with b:
        p = dec[3]
        src = pinned_rgb(b, fx, p, 3)
        for aa in (True, False):
            want = reference(src, kw["size"], kw.get("crop"), aa)
            check(b.tensor([p], antialias=aa, **kw).cpu()[0], want, torch.float32)
            t = as_nchw(b.tensor([p], antialias=aa, dtype=torch.uint8, layout="nhwc", **kw), "nhwc").cpu()[0]
            check(t, reference(src, kw["size"], kw.get("crop"), aa, u8=True), torch.uint8)


# ------------------------------------------------------------------------------------------------------ gather, out=

def test_gather_repeats_reverse_and_all():
    fx, es = load("coherent_pan_352x288")
    b, dec = decoded_batch(fx, es)
    with b:
        assert dec == list(range(b.picture_count))
        order = [7, 7, 3, 0, 11, 3] + list(range(b.picture_count))[::-1]
        src = {p: pinned_rgb(b, fx, p, p) for p in set(order)}
        t = b.tensor(order, size=(100, 120)).cpu()
        for k, p in enumerate(order):
            check(t[k], reference(src[p], (100, 120)), torch.float32)
        allp = b.tensor(None, size=(100, 120)).cpu()
        assert allp.shape[0] == b.picture_count
        assert torch.equal(allp, t[6:].flip(0))
        assert torch.equal(b.tensor(np.array(order, dtype=np.int64), size=(100, 120)).cpu(), t)
        assert torch.equal(b.tensor(range(3), size=(100, 120)).cpu(), allp[:3])


def test_out_slice_and_bad_out():
    fx, es = load("coherent_pan_352x288")
    b, dec = decoded_batch(fx, es)
    with b:
        big = torch.full((6, 3, 64, 80), 7.0, dtype=torch.float16, device="cuda:0")
        r = b.tensor([2, 9], size=(64, 80), dtype=torch.float16, out=big[2:4])
        assert r.data_ptr() == big[2:4].data_ptr()
        ref = b.tensor([2, 9], size=(64, 80), dtype=torch.float16)
        torch.cuda.synchronize()
        assert torch.equal(big[2:4], ref)
        assert bool((big[:2] == 7).all()) and bool((big[4:] == 7).all())
        for bad in (torch.empty((2, 3, 64, 81), dtype=torch.float16, device="cuda:0"),                 # shape
                    torch.empty((2, 3, 64, 80), dtype=torch.float32, device="cuda:0"),                 # dtype
                    torch.empty((2, 3, 64, 80), dtype=torch.float16),                                  # device
                    torch.empty((2, 3, 64, 160), dtype=torch.float16, device="cuda:0")[..., ::2],      # stride
                    torch.empty((2, 64, 80, 3), dtype=torch.float16, device="cuda:0")):                # layout
            with pytest.raises(ValueError):
                b.tensor([2, 9], size=(64, 80), dtype=torch.float16, out=bad)


# ------------------------------------------------------------------------------------------------------ stream order

SLEEP = 200_000_000          # torch.cuda._sleep cycles in front of a render: tens of milliseconds


def test_pool_ready_event_orders_a_render_after_an_unsynchronised_decode():
    fx, es = load("cfg2_1080p")
    fx_old, es_old = load("enc1080_2")
    n, per = 64, fx["n_frames"]
    # the deepest pictures (dependency level 11 of a GOP of 12) of 32 of the 64 streams: reconstructed by the LAST launches
    deep = [s * per + k for s in range(0, n, 2) for k in (11, 23)]
    with jb.Batch(1920, 1080, n, (per + 2) * n, (len(es) + 1024) * n, device=0) as ref_b:       # the reference pictures
        ref_b.upload([es] * n)
        ref_b.decode()
        assert sum(1 for i in ref_b.pictures() if i.decoded) == per * n
        want = [reference(pinned_rgb(ref_b, fx, p, p % per), (64, 64)) for p in deep]
    n_old = -(-(per * n) // fx_old["n_frames"])              # copies of another 1080p GOP: they fill every slot `deep` goes to
    pool = max(n_old * (fx_old["n_frames"] + 2), (per + 2) * n)
    with jb.Batch(1920, 1080, max(n, n_old), pool, max(len(es) * n, len(es_old) * n_old) + 1024 * max(n, n_old), device=0) as b:
        b.set_reconstruct("levels")
        b.upload([es_old] * n_old)
        # the decode on a stream of its own (work on the null stream orders later launches behind it by itself), the render on
        # one of higher priority (a hardware queue of its own: one shared with the decode's would run behind it anyway); both
        # streams used once before, every slot-table stage allocated and the output too -- a stream's first launch and an
        # allocation can take milliseconds, and the race would be over by then
        d, s = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0, priority=-1)
        b.decode(stream=d.cuda_stream)                      # synchronised: the pool holds the OTHER pictures where `deep` goes
        old = b.tensor(deep, size=(64, 64)).cpu()
        out = torch.empty((len(deep), 3, 64, 64), device="cuda:0")
        with torch.cuda.stream(s):
            for _ in range(4):
                b.tensor(deep, size=(64, 64), out=out)
        torch.cuda.synchronize()
        for k in range(len(deep)):
            assert float((old[k] - want[k]).abs().max()) > 0.1, "the pool must hold other pictures before the decode"
        b.upload([es] * n)
        # level by level the host waits for the index and for the parse's coverage counts (ev_cov), not for the reconstruct:
        # when decode returns, the launches of dependency levels 1 .. 11 (128 pictures each) are still queued on the decode stream
        b.decode(stream=d.cuda_stream, sync=False)          # (the deepest levels finish about 2.5 ms after this returns)
        with torch.cuda.stream(s):
            t = b.tensor(deep, size=(64, 64), out=out)
        s.synchronize()
        t = t.cpu()
        for k in range(len(deep)):
            check(t[k], want[k], torch.float32)


def test_pool_read_event_holds_the_next_decode():
    fx0, es0 = load("enc1080_0")
    fx1, es1 = load("enc1080_2")
    with jb.Batch(1920, 1080, 1, 64, max(len(es0), len(es1)) + 4096, device=0) as b:
        b.set_reconstruct("levels")
        b.upload([es0])
        b.decode()
        pics = [p for p, i in enumerate(b.pictures()) if i.decoded][:6]
        want = [reference(pinned_rgb(b, fx0, p, k), (224, 224)) for k, p in enumerate(pics)]
        s = torch.cuda.Stream(device=0)
        with torch.cuda.stream(s):
            torch.cuda._sleep(SLEEP)
            t = b.tensor(pics, size=(224, 224))
        b.upload([es1])                                      # at once: no synchronise
        b.decode(sync=False)
        b.sync()
        s.synchronize()
        other = [reference(pinned_rgb(b, fx1, p, k), (224, 224)) for k, p in enumerate(pics)]
        for k in range(len(pics)):
            assert float((other[k] - want[k]).abs().max()) > 0.1, "the second batch's pictures must differ from the first's"
            check(t[k].cpu(), want[k], torch.float32)


def test_enqueued_pass_is_settled_first():
    fx, es = load("cfg1_720p")
    with jb.Batch(1280, 720, 2, (fx["n_frames"] + 2) * 2, (len(es) + 1024) * 2, device=0) as b:
        b.upload([es, es])
        b.enqueue()
        t = b.tensor([0, 1, 5], size=(224, 224), dtype=torch.bfloat16)
        dec = [p for p, i in enumerate(b.pictures()) if i.decoded]
        assert dec[:6] == list(range(6))
        for k, p in enumerate([0, 1, 5]):
            check(t[k].cpu(), reference(pinned_rgb(b, fx, p, p), (224, 224)), torch.bfloat16)


# ------------------------------------------------------------------------------------------------------------- live

def picture_writes(es, offs):
    n = len(offs) - 1
    return [es[int(offs[k]):(len(es) if k == n - 1 else int(offs[k + 1]))] for k in range(n)]


def live_ref(lv, i, fx=None, size=(96, 120)):
    y, cr, cb = lv.read_frame(i)
    return reference(rgb(*planes(np.concatenate([y, cr, cb]), lv.coded_width, lv.coded_height), lv.width, lv.height), size)


def test_live_tensor_and_latest_tensor():
    fx = json.load(open(os.path.join(GOLDEN, "frames_coherent_pan_352x288.json")))
    es, offs = synth.generate_config(fx["config"], n_frames=fx["n_frames"], **fx["overrides"])
    writes = picture_writes(es, offs)
    with jl.Live(352, 288, 8, pictures_per_tick=2, store_bytes=1 << 18, device=0) as lv:
        ids = [lv.open() for _ in range(8)]
        seen = {i: 0 for i in ids}
        latest = {}
        # tick 1: streams 0-5 two pictures each; tick 2: streams 0-2 one more; stream 6 and 7 never written
        for t, streams, per in ((1, ids[:6], 2), (2, ids[:3], 1)):
            for i in streams:
                for _ in range(per):
                    lv.write(i, writes[seen[i]]); seen[i] += 1
            n = lv.tick(flush=True)
            pics = lv.pictures()
            assert n == len(pics) == len(streams) * per
            for q, pic in enumerate(pics):
                assert md5_planes(*lv.read_frame(q)) == fx["frame_md5"][seen[pic.stream] - per + sum(1 for r in pics[:q] if r.stream == pic.stream)]
            want = [live_ref(lv, q) for q in range(n)]
            got = lv.tensor(size=(96, 120)).cpu()
            rev = lv.tensor(list(range(n))[::-1], size=(96, 120), dtype=torch.float16).cpu()
            for q in range(n):
                check(got[q], want[q], torch.float32)
                check(rev[n - 1 - q], want[q], torch.float16)
                latest[pics[q].stream] = want[q]
        t, have = lv.latest_tensor(ids, size=(96, 120))
        assert have.tolist() == [i in latest for i in ids] == [True] * 6 + [False] * 2
        t = t.cpu()
        for k, i in enumerate(ids):
            if i in latest:
                check(t[k], latest[i], torch.float32)
            else:
                assert bool((t[k] == 0).all())
        with pytest.raises(RuntimeError, match="not open"):
            lv.latest_tensor([0, 99], size=(96, 120))
        with pytest.raises(RuntimeError, match="outside"):
            lv.tensor([0, 3], size=(96, 120))


def test_live_tick_waits_for_a_delayed_render():
    fx = json.load(open(os.path.join(GOLDEN, "frames_coherent_pan_352x288.json")))
    es, offs = synth.generate_config(fx["config"], n_frames=fx["n_frames"], **fx["overrides"])
    writes = picture_writes(es, offs)
    with jl.Live(352, 288, 2, pictures_per_tick=2, store_bytes=1 << 18, device=0) as lv:
        a = lv.open()
        k = 0
        for _ in range(2):
            lv.write(a, writes[k]); k += 1
        assert lv.tick(flush=True) == 1 + 1
        want_tick = [live_ref(lv, q) for q in range(2)]
        want_latest = want_tick[1]
        s = torch.cuda.Stream(device=0)
        with torch.cuda.stream(s):
            torch.cuda._sleep(SLEEP)
            got_tick = lv.tensor(size=(96, 120))
            got_latest, have = lv.latest_tensor([a], size=(96, 120))
        for _ in range(2):                                  # two ticks of two pictures: the ring (4 frames) comes round
            for _ in range(2):
                lv.write(a, writes[k]); k += 1
            assert lv.tick(flush=True) == 2
        s.synchronize()
        assert have.tolist() == [True]
        check(got_latest[0].cpu(), want_latest, torch.float32)
        for q in range(2):
            check(got_tick[q].cpu(), want_tick[q], torch.float32)


# ------------------------------------------------------------------------------------------------------- rejections

def test_rejections_change_no_output_byte():
    fx, es = load("skipped_pictures_352x288")
    w, h = fx["info"]["width"], fx["info"]["height"]
    with jb.Batch(w, h, 1, len(fx["abi_frame_md5"]) + 2, len(es) + 1024, device=0) as b:
        b.upload([es])
        b.decode()
        info = b.pictures()
        skipped = [p for p, i in enumerate(info) if not i.decoded]
        good = [p for p, i in enumerate(info) if i.decoded]
        assert skipped
        out = torch.full((2, 3, 32, 32), 0.25, device="cuda:0")
        for pics, kw, msg in (([good[0], skipped[0]], {}, "not decoded"),
                              ([good[0], len(info)], {}, "outside"),
                              ([good[0], good[1]], dict(crop=(300, 0, 100, 10)), "crop"),
                              ([good[0], good[1]], dict(crop=(0, 0, 10, 0)), "crop")):
            with pytest.raises(RuntimeError, match=msg):
                b.tensor(pics, size=(32, 32), out=out, **kw)
        torch.cuda.synchronize()
        assert bool((out == 0.25).all())
        with pytest.raises(RuntimeError, match="not decoded"):
            b.tensor(None, size=(32, 32))
        assert b.tensor([], size=(32, 32)).shape == (0, 3, 32, 32)
