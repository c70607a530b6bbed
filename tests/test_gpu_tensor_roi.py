"""Tensor rows from regions of interest on the GPU (Batch.tensor_rois, Live.tensor_rois, Live.latest_tensor_rois ->
k_tensor_roi).  Two sources of truth: every row must equal, bit for bit, what Batch.tensor gives for its picture with
crop = the clipped box; and the rows pass tensor_ref.check against the host's reference (numpy integer RGB of the planes,
pinned to the golden md5s first; torch's CPU resize), which tests/test_tensor_roi_plan.py holds the CPU simulator to for
the same box lists (tests/tensor_roi_inputs.py)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import tensor_roi_inputs as ri
from jsmpeg_amd import batch as jb, live as jl, synth, tensor as jt
from tensor_ref import DTYPES, IMAGENET_MEAN, IMAGENET_STD, check, planes, reference, rgb
from test_gpu_tensor import GOLDEN, SLEEP, decoded_batch, load, picture_writes, pinned_rgb

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def rois_dev(rois):
    return torch.tensor([list(r) for r in rois], dtype=torch.int32, device=DEV).reshape(-1, 5)


class Pan:
    """coherent_pan_352x288 decoded once for the module: the batch, and each picture's integer RGB (planes pinned first)"""

    def __init__(self):
        self.fx, es = load("coherent_pan_352x288")
        self.b, dec = decoded_batch(self.fx, es)
        assert dec == list(range(self.b.picture_count)) and (self.b.width, self.b.height) == (ri.W, ri.H)
        self._src, self._ref = {}, {}

    def src(self, p):
        if p not in self._src:
            self._src[p] = pinned_rgb(self.b, self.fx, p, p)
        return self._src[p]

    def ref(self, p, box, size, aa, u8=False):
        key = (p, tuple(box), tuple(size), bool(aa), u8)
        if key not in self._ref:
            self._ref[key] = reference(self.src(p), size, box, aa, u8=u8)
        return self._ref[key]


@pytest.fixture(scope="module")
def pan():
    p = Pan()
    yield p
    p.b.close()


def as_nchw(t, layout):
    return t.permute(0, 3, 1, 2) if layout == "nhwc" else t


def is_zero(t):
    return not bool(t.contiguous().view(torch.uint8).any())


def compare_mixed(pan, t, status, size, aa):
    """f32 NCHW RGB rows of ri.MIXED: bit-equal to Batch.tensor(crop=), and the reference under check"""
    assert status.tolist() == [ri.INSIDE] * len(ri.MIXED)
    tc = t.cpu()
    for r, roi in enumerate(ri.MIXED):
        p = ri.MIXED_PICTURES[roi[0]]
        assert torch.equal(t[r], pan.b.tensor([p], size=size, crop=roi[1:], antialias=aa)[0]), (r, roi)
        check(tc[r], pan.ref(p, roi[1:], size, aa), torch.float32)


# ------------------------------------------------------------------------------------------ 1. mixed boxes in one call

@pytest.mark.parametrize("aa", [True, False], ids=["aa", "plain"])
@pytest.mark.parametrize("size", ri.SIZES, ids=["%dx%d" % (s[1], s[0]) for s in ri.SIZES])
def test_mixed_boxes_in_one_call(pan, size, aa):
    b, pics, rois = pan.b, list(ri.MIXED_PICTURES), rois_dev(ri.MIXED)
    n = len(ri.MIXED)
    for dname, dt in DTYPES.items():
        for layout in ("nchw", "nhwc"):
            for order in ("rgb", "bgr"):
                kw = dict(size=size, dtype=dt, layout=layout, order=order, antialias=aa)
                if order == "bgr":
                    kw.update(mean=IMAGENET_MEAN[::-1], std=IMAGENET_STD[::-1])
                t, status = b.tensor_rois(rois, pics, **kw)
                assert t.shape == ((n, 3) + tuple(size) if layout == "nchw" else (n,) + tuple(size) + (3,))
                assert t.dtype == dt and t.is_contiguous() and t.device == torch.device(DEV)
                assert status.dtype == torch.uint8 and status.device == t.device and status.tolist() == [ri.INSIDE] * n
                one = {}
                for r, roi in enumerate(ri.MIXED):
                    if roi not in one:
                        one[roi] = b.tensor([pics[roi[0]]], crop=roi[1:], **kw)[0]
                    assert torch.equal(t[r], one[roi]), "%s %s %s row %d %r differs from Batch.tensor(crop=)" % (dname, layout, order, r, roi)
                if order == "rgb" and (dt != torch.uint8 or tuple(size) == ri.U8_CHECK_SIZE):
                    tc = as_nchw(t, layout).cpu()
                    for r, roi in enumerate(ri.MIXED):
                        check(tc[r], pan.ref(pics[roi[0]], roi[1:], size, aa, u8=dt == torch.uint8), dt)


# -------------------------------------------------------------------------------------------------------- 2. identity

def test_identity_box_is_the_pinned_rgb(pan):
    for box in ri.BOXES12:
        size = (box[3], box[2])
        if size not in ri.SIZES:
            continue
        rois = rois_dev([(k,) + box for k in range(3)])
        for layout in ("nchw", "nhwc"):
            t, status = pan.b.tensor_rois(rois, [3, 6, 10], size=size, dtype=torch.uint8, layout=layout)
            assert status.tolist() == [ri.INSIDE] * 3
            t = as_nchw(t, layout).cpu().numpy()
            for k, p in enumerate((3, 6, 10)):
                assert np.array_equal(t[k], pan.src(p)[:, box[1]:box[1] + box[3], box[0]:box[0] + box[2]]), (box, layout, p)


# --------------------------------------------------------------------------------------- 3. many taps, narrow chunks

@pytest.mark.parametrize("case", sorted(ri.MANY_TAPS))
def test_many_taps_narrow_chunks(pan, case):
    fixture, box, size = ri.MANY_TAPS[case]
    if fixture == "coherent_pan_352x288":
        b, src, p = pan.b, pan.src(3), 3
    else:
        fx, es = load(fixture)
        b, dec = decoded_batch(fx, es)
        p = dec[3]
        src = pinned_rgb(b, fx, p, 3)
    try:
        rois = rois_dev([(0,) + box])
        for aa in (True, False):
            t, status = b.tensor_rois(rois, [p], size=size, antialias=aa)
            assert status.tolist() == [ri.INSIDE]
            assert torch.equal(t, b.tensor([p], size=size, crop=box, antialias=aa))
            check(t[0].cpu(), reference(src, size, box, aa), torch.float32)
    finally:
        if b is not pan.b:
            b.close()


# ------------------------------------------------------------------------------------ 4. bad boxes beside good ones

@pytest.mark.parametrize("dname,size", [("f16", ri.SIZES[0]), ("f32", ri.SIZES[1]), ("u8", ri.SIZES[1])])
def test_bad_boxes_beside_good_ones(pan, dname, size):
    b, pics, dt = pan.b, list(ri.BAD_PICTURES), DTYPES[dname]
    n = len(ri.BAD)
    want = [ri.clip(r, len(pics), ri.W, ri.H) for r in ri.BAD]
    assert {s for s, _ in want} == {ri.EMPTY, ri.INSIDE, ri.CLIPPED}
    big = torch.full((n + 5, 3) + tuple(size), 7, dtype=dt, device=DEV)
    t, status = b.tensor_rois(rois_dev(ri.BAD), pics, size=size, dtype=dt, out=big[2:2 + n])
    assert t.data_ptr() == big[2:2 + n].data_ptr()
    assert status.tolist() == [s for s, _ in want]
    assert bool((big[:2] == 7).all()) and bool((big[2 + n:] == 7).all()), "rows outside the slice were written"
    tc = t.cpu()
    for r, (st, box) in enumerate(want):
        if st == ri.EMPTY:
            assert is_zero(t[r]), (r, ri.BAD[r])
            continue
        p = pics[ri.BAD[r][0]]
        assert torch.equal(t[r], b.tensor([p], size=size, crop=box, dtype=dt)[0]), (r, ri.BAD[r], box)
        check(tc[r], pan.ref(p, box, size, True, u8=dt == torch.uint8), dt)


# ------------------------------------------------------------------------- 5. more rows than the grid's y limit

def test_more_rows_than_the_grid_y_limit(pan):
    b, pics = pan.b, list(ri.CYCLE_PICTURES)
    n, c = ri.CYCLE_ROWS, len(ri.CYCLE16)
    assert n > 65535 and n % c != 0
    rois = rois_dev(ri.CYCLE16).repeat(n // c + 1, 1)[:n].contiguous()
    t, status = b.tensor_rois(rois, pics, size=ri.CYCLE_SIZE, dtype=torch.uint8)
    assert t.shape == (n, 3) + ri.CYCLE_SIZE and status.shape == (n,)
    assert bool((status == ri.INSIDE).all())
    full = (n // c) * c
    assert torch.equal(t[:full].view(n // c, c, -1), t[:c].view(1, c, -1).expand(n // c, c, -1)), "row r differs from row r % 16"
    assert torch.equal(t[full:], t[:n - full])
    for r, roi in enumerate(ri.CYCLE16):
        assert torch.equal(t[r], b.tensor([pics[roi[0]]], size=ri.CYCLE_SIZE, crop=roi[1:], dtype=torch.uint8)[0]), (r, roi)


# ------------------------------------------------------------------------------------------- 6. device-made boxes

def test_device_made_boxes_need_no_synchronise(pan):
    size, aa = ri.SIZES[1], True
    m = torch.tensor([list(r) for r in ri.MIXED], dtype=torch.float32, device=DEV)
    rows_host = torch.tensor([r[0] for r in ri.MIXED], device=DEV)
    inset = torch.tensor([0.3, 0.6, -0.2, -0.7], device=DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=0)
    with torch.cuda.stream(s):
        torch.cuda._sleep(SLEEP)                           # the boxes do not exist yet when the call is made
        xyxy = torch.stack([m[:, 1], m[:, 2], m[:, 1] + m[:, 3], m[:, 2] + m[:, 4]], dim=1) + inset
        rois = jt.rois_from_xyxy(xyxy / 2, rows_host, scale=(2, 2))
        assert rois.dtype == torch.int32 and rois.device == m.device
        t, status = pan.b.tensor_rois(rois, list(ri.MIXED_PICTURES), size=size, antialias=aa)
    s.synchronize()
    assert rois.tolist() == [list(r) for r in ri.MIXED]
    compare_mixed(pan, t, status, size, aa)


# ------------------------------------------------------------------------------------------------------------ 7. live

def live_rgb(lv, i):
    y, cr, cb = lv.read_frame(i)
    return rgb(*planes(np.concatenate([y, cr, cb]), lv.coded_width, lv.coded_height), lv.width, lv.height)


def pan_writes():
    fx = json.load(open(os.path.join(GOLDEN, "frames_coherent_pan_352x288.json")))
    es, offs = synth.generate_config(fx["config"], n_frames=fx["n_frames"], **fx["overrides"])
    return picture_writes(es, offs)


def test_live_tensor_rois_and_latest_tensor_rois():
    writes = pan_writes()
    size = ri.SIZES[1]
    with jl.Live(352, 288, 4, pictures_per_tick=2, store_bytes=1 << 18, device=0) as lv:
        ids = [lv.open() for _ in range(3)]
        for k in range(2):                                  # streams 0 and 1 two pictures each; stream 2 never written
            for i in ids[:2]:
                lv.write(i, writes[k])
        n = lv.tick(flush=True)
        pics = lv.pictures()
        assert n == len(pics) == 4
        src = [live_rgb(lv, q) for q in range(n)]
        boxes = ri.BOXES12[:8]
        rois = [(q % n,) + box for q, box in enumerate(boxes)]
        t, status = lv.tensor_rois(rois_dev(rois), size=size)
        assert status.tolist() == [ri.INSIDE] * len(rois)
        for r, roi in enumerate(rois):
            assert torch.equal(t[r], lv.tensor([roi[0]], size=size, crop=roi[1:])[0]), (r, roi)
            check(t[r].cpu(), reference(src[roi[0]], size, roi[1:]), torch.float32)
        # a picture list of its own, reversed: row 0 is the tick's last picture
        t2, _ = lv.tensor_rois(rois_dev(rois), list(range(n))[::-1], size=size)
        for r, roi in enumerate(rois):
            check(t2[r].cpu(), reference(src[n - 1 - roi[0]], size, roi[1:]), torch.float32)
        newest = {}
        for q, pic in enumerate(pics):
            newest[pic.stream] = q                           # (a stream's pictures come in order)
        lrois = [(k % 3,) + box for k, box in enumerate(boxes)]
        t, status, have = lv.latest_tensor_rois(rois_dev(lrois), ids, size=size)
        assert have.tolist() == [True, True, False]
        assert status.tolist() == [ri.EMPTY if roi[0] == 2 else ri.INSIDE for roi in lrois]
        for r, roi in enumerate(lrois):
            if roi[0] == 2:
                assert is_zero(t[r]), (r, roi)
            else:
                check(t[r].cpu(), reference(src[newest[ids[roi[0]]]], size, roi[1:]), torch.float32)
                assert torch.equal(t[r], lv.latest_tensor([ids[roi[0]]], size=size, crop=roi[1:])[0][0]), (r, roi)
        with pytest.raises(RuntimeError, match="not open"):
            lv.latest_tensor_rois(rois_dev(lrois), [0, 99], size=size)
        with pytest.raises(RuntimeError, match="outside"):
            lv.tensor_rois(rois_dev(rois), [0, 4], size=size)
        t, status, have = lv.latest_tensor_rois(rois_dev([]), ids, size=size)
        assert t.shape == (0, 3) + size and status.shape == (0,) and have.tolist() == [True, True, False]


def test_live_tick_waits_for_a_delayed_roi_render():
    writes = pan_writes()
    size = ri.SIZES[1]
    with jl.Live(352, 288, 2, pictures_per_tick=2, store_bytes=1 << 18, device=0) as lv:
        a = lv.open()
        k = 0
        for _ in range(2):
            lv.write(a, writes[k]); k += 1
        assert lv.tick(flush=True) == 2
        src = [live_rgb(lv, q) for q in range(2)]
        rois = [(q % 2,) + box for q, box in enumerate(ri.BOXES12[:6])]
        lrois = [(0,) + box for box in ri.BOXES12[:6]]
        d_rois, d_lrois = rois_dev(rois), rois_dev(lrois)
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device=0)
        with torch.cuda.stream(s):
            torch.cuda._sleep(SLEEP)
            got_tick, st_tick = lv.tensor_rois(d_rois, size=size)
            got_latest, st_latest, have = lv.latest_tensor_rois(d_lrois, [a], size=size)
        for _ in range(2):                                  # two ticks of two pictures: the ring (4 frames) comes round
            for _ in range(2):
                lv.write(a, writes[k]); k += 1
            assert lv.tick(flush=True) == 2
        s.synchronize()
        assert have.tolist() == [True] and st_tick.tolist() == [ri.INSIDE] * 6 and st_latest.tolist() == [ri.INSIDE] * 6
        for r in range(6):
            check(got_tick[r].cpu(), reference(src[rois[r][0]], size, rois[r][1:]), torch.float32)
            check(got_latest[r].cpu(), reference(src[1], size, lrois[r][1:]), torch.float32)


# ---------------------------------------------------------------------------------------------- 8. host-visible errors

def test_host_visible_errors_change_no_output_byte():
    fx, es = load("skipped_pictures_352x288")
    w, h = fx["info"]["width"], fx["info"]["height"]
    with jb.Batch(w, h, 1, len(fx["abi_frame_md5"]) + 2, len(es) + 1024, device=0) as b:
        b.upload([es])
        b.decode()
        info = b.pictures()
        skipped = [p for p, i in enumerate(info) if not i.decoded]
        good = [p for p, i in enumerate(info) if i.decoded]
        assert skipped
        rois = rois_dev([(0, 0, 0, 50, 50), (1, 10, 10, 50, 50)])
        out = torch.full((2, 3, 32, 32), 0.25, device=DEV)
        for pics, msg in (([good[0], skipped[0]], "not decoded"), ([good[0], len(info)], "outside")):
            with pytest.raises(RuntimeError, match=msg):
                b.tensor_rois(rois, pics, size=(32, 32), out=out)
        with pytest.raises(RuntimeError, match="not decoded"):
            b.tensor_rois(rois, None, size=(32, 32), out=out)
        # a descriptor with a crop of its own: the Python call has no such argument, so through the C ABI
        pics = np.array(good[:2], dtype=np.uint32)
        for crop in ((0, 0, 10, 10), (3, 0, 0, 0)):
            d = jt.TensorDesc(32, 32, *crop, jt.F32, jt.NCHW, jt.RGB, 1, (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1))
            rc = b.L.jsmpeg_hip_batch_render_tensor_rois(b.h, pics.ctypes.data, 2, ctypes.byref(d), rois.data_ptr(), 2, out.data_ptr(),
                                                          None, torch.cuda.current_stream().cuda_stream)
            assert rc < 0 and "crop and rois exclude each other" in jb.last_error()
        with pytest.raises(ValueError, match="size"):
            b.tensor_rois(rois, good[:2], out=out)
        with pytest.raises(ValueError, match="size"):
            b.tensor_rois(rois, good[:2], size=(32, 4097), out=out)
        for bad in (torch.empty((3, 3, 32, 32), device=DEV),                                  # rows
                    torch.empty((2, 3, 32, 33), device=DEV),                                  # shape
                    torch.empty((2, 3, 32, 32), dtype=torch.float16, device=DEV),             # dtype
                    torch.empty((2, 3, 32, 32)),                                              # device
                    torch.empty((2, 3, 32, 64), device=DEV)[..., ::2],                        # stride
                    torch.empty((2, 32, 32, 3), device=DEV)):                                 # layout
            with pytest.raises(ValueError, match="out"):
                b.tensor_rois(rois, good[:2], size=(32, 32), out=bad)
        for bad in (torch.zeros((2, 4), dtype=torch.int32, device=DEV), torch.zeros((2, 5), device=DEV), [[0.5, 0, 0, 8, 8]],
                    [[0, 0, 0, 8, 1 << 31]]):
            with pytest.raises(ValueError, match="rois"):
                b.tensor_rois(bad, good[:2], size=(32, 32), out=out)
        torch.cuda.synchronize()
        assert bool((out == 0.25).all())
        # the good call writes it; a host list of boxes is copied to the device
        t, status = b.tensor_rois([(0, 0, 0, 50, 50), (1, 10, 10, 50, 50)], good[:2], size=(32, 32), out=out)
        assert status.tolist() == [ri.INSIDE] * 2 and torch.equal(out[1], b.tensor([good[1]], size=(32, 32), crop=(10, 10, 50, 50))[0])
        for empty in (torch.empty((0, 5), dtype=torch.int32, device=DEV), []):
            t, status = b.tensor_rois(empty, good[:2], size=(32, 32))
            assert t.shape == (0, 3, 32, 32) and status.shape == (0,) and status.dtype == torch.uint8
