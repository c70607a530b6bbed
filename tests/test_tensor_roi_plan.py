"""Tensor rows from regions of interest without a GPU: tensor_plan.h's clip rule and per-row plan -- what k_tensor_roi
(kernels.hip) runs -- compiled by g++ into a TEST-ONLY simulator (tests/sim/sim_tensor_roi.cpp) and held against
tensor_ref.reference of the clipped box for every box list the GPU tests use (tests/tensor_roi_inputs.py); the Python helper
rois_from_xyxy; the library's exports and the kernel's resources."""
import ctypes
import glob
import os
import subprocess

import numpy as np
import pytest
import torch

import tensor_roi_inputs as ri
from conftest import ROOT
from tensor_ref import check, planes, reference, rgb
from test_tensor_plan import Desc, desc, random_frame

CSRC = os.path.join(ROOT, "jsmpeg_amd", "csrc")


@pytest.fixture(scope="module")
def sim():
    so = os.path.join(ROOT, "tests", "sim", "libjsmpeg_sim_tensor_roi.so")
    src = os.path.join(ROOT, "tests", "sim", "sim_tensor_roi.cpp")
    deps = [src] + glob.glob(os.path.join(CSRC, "*.h")) + [os.path.join(ROOT, "include", "jsmpeg_hip.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-I", CSRC,
                               "-I", os.path.join(ROOT, "include"), "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    lib.sim_roi_clip.restype = ctypes.c_int
    lib.sim_roi_clip.argtypes = [vp, u32, u32, u32, vp]
    lib.sim_tensor_roi_check.restype = ctypes.c_char_p
    lib.sim_tensor_roi_check.argtypes = [ctypes.POINTER(Desc), u32, u32]
    lib.sim_tensor_rois.restype = ctypes.c_int
    lib.sim_tensor_rois.argtypes = [vp, vp, u32, u32, u32, u32, u32, ctypes.POINTER(Desc), vp, u32, vp, vp]
    return lib


def sim_clip(sim, roi, count, w, h):
    r = np.array(roi, dtype=np.int32)
    out = np.zeros(4, dtype=np.int32)
    st = sim.sim_roi_clip(r.ctypes.data, count, w, h, out.ctypes.data)
    return st, (tuple(int(v) for v in out) if st else None)


def run_sim(sim, frames, present, cw, ch, w, h, d, rois):
    """frames [count][cw * ch * 3 / 2] -> (rows [R][3][oh][ow] float32 torch, status [R])"""
    rois = np.ascontiguousarray(rois, dtype=np.int32).reshape(-1, 5)
    present = np.ascontiguousarray(present, dtype=np.uint8)
    out = np.full((len(rois), 3, d.height, d.width), -7.0, dtype=np.float32)
    status = np.full(len(rois), 9, dtype=np.uint8)
    assert sim.sim_tensor_rois(frames.ctypes.data, present.ctypes.data, len(frames), cw, ch, w, h, ctypes.byref(d),
                               rois.ctypes.data, len(rois), out.ctypes.data, status.ctypes.data) == 0
    return torch.from_numpy(out), status


# --------------------------------------------------------------------------------------------------------- the rule

E = ri.I32_MAX
CLIP_CASES = {
    "inside": ((1, 33, 21, 120, 90), 3),
    "whole": ((0, 0, 0, ri.W, ri.H), 1),
    "one_pixel_last": ((0, ri.W - 1, ri.H - 1, 1, 1), 1),
    "over_left": ((0, -10, 50, 100, 60), 1), "over_top": ((0, 50, -7, 100, 60), 1),
    "over_right": ((0, 300, 50, 100, 60), 1), "over_bottom": ((0, 50, 250, 100, 60), 1),
    "over_all": ((0, -5, -5, 400, 300), 1),
    "out_left": ((0, -100, 50, 100, 60), 1), "out_right": ((0, ri.W, 50, 10, 10), 1),
    "out_top": ((0, 50, -60, 100, 60), 1), "out_bottom": ((0, 50, ri.H, 10, 10), 1),
    "zero_w": ((0, 10, 10, 0, 10), 1), "zero_h": ((0, 10, 10, 10, 0), 1),
    "neg_w": ((0, 10, 10, -5, 10), 1), "neg_h": ((0, 10, 10, 10, -1), 1), "min_size": ((0, 10, 10, ri.I32_MIN, ri.I32_MIN), 1),
    "row_m1": ((-1, 0, 0, 8, 8), 3), "row_count": ((3, 0, 0, 8, 8), 3), "row_last": ((2, 0, 0, 8, 8), 3),
    "row_min": ((ri.I32_MIN, 0, 0, 8, 8), 3), "row_max": ((E, 0, 0, 8, 8), 3), "no_pictures": ((0, 0, 0, 8, 8), 0),
    "max_max": ((0, E, E, E, E), 1), "min_max": ((0, ri.I32_MIN, ri.I32_MIN, E, E), 1),
    "m1_max": ((0, -1, -1, E, E), 1), "zero_max": ((0, 0, 0, E, E), 1),
    "ends_at_0": ((0, -E, 100, E, 50), 1), "ends_at_1": ((0, -E + 1, 100, E, 50), 1),
    "x_max_w_1": ((0, E, 0, 1, 1), 1), "y_min": ((0, 0, ri.I32_MIN, 8, E), 1),
}


@pytest.mark.parametrize("case", sorted(CLIP_CASES))
def test_roi_clip_is_the_stated_rule(sim, case):
    roi, count = CLIP_CASES[case]
    want = ri.clip(roi, count, ri.W, ri.H)
    assert sim_clip(sim, roi, count, ri.W, ri.H) == want
    if want[0]:
        x, y, bw, bh = want[1]
        assert 0 <= x and 0 <= y and bw >= 1 and bh >= 1 and x + bw <= ri.W and y + bh <= ri.H


def test_roi_clip_expected_statuses():
    """the Python restatement itself, on cases whose answer is plain"""
    assert ri.clip((0, 33, 21, 120, 90), 1, ri.W, ri.H) == (ri.INSIDE, (33, 21, 120, 90))
    assert ri.clip((0, 300, 50, 100, 60), 1, ri.W, ri.H) == (ri.CLIPPED, (300, 50, 52, 60))
    assert ri.clip((0, -5, -5, 400, 300), 1, ri.W, ri.H) == (ri.CLIPPED, (0, 0, ri.W, ri.H))
    assert ri.clip((0, E, E, E, E), 1, ri.W, ri.H) == (ri.EMPTY, None)
    assert ri.clip((0, -E + 1, 100, E, 50), 1, ri.W, ri.H) == (ri.CLIPPED, (0, 100, 1, 50))
    assert ri.clip((1, 0, 0, 8, 8), 1, ri.W, ri.H) == (ri.EMPTY, None)
    assert [ri.clip(r, 3, ri.W, ri.H)[0] for r in ri.BAD] == [1, 2, 2, 2, 2, 2, 1] + [0] * 9 + [1] + [0] * 6 + [2, 2, 0, 0, 2, 1]
    assert all(ri.clip(r, 3, ri.W, ri.H)[0] == ri.INSIDE for r in ri.MIXED + ri.CYCLE16)


def test_descriptor_with_a_crop_is_refused(sim):
    for crop in ((0, 0, 10, 10), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 0, 5)):
        assert "exclude" in sim.sim_tensor_roi_check(ctypes.byref(desc(8, 8, crop)), ri.W, ri.H).decode()
    assert sim.sim_tensor_roi_check(ctypes.byref(desc(8, 8)), ri.W, ri.H).decode() == ""
    assert "dtype" in sim.sim_tensor_roi_check(ctypes.byref(desc(8, 8, dtype=4)), ri.W, ri.H).decode()


# ------------------------------------------------------------------------------------------- the rows against torch

@pytest.fixture(scope="module")
def frames352():
    f = np.stack([random_frame(ri.W, ri.H, 100 + k) for k in range(3)])
    return f, [rgb(*planes(f[k], ri.W, ri.H), ri.W, ri.H) for k in range(3)]


def check_rows(sim, frames, src, cw, ch, w, h, rois, size, aa, present=None):
    """every row of the list: f32 (and that value cast to f16 and bf16) under check; u8 too from U8_CHECK_SIZE up; status and
    zero rows by the rule"""
    oh, ow = size
    present = [1] * len(frames) if present is None else present
    got, status = run_sim(sim, frames, present, cw, ch, w, h, desc(ow, oh, aa=aa), rois)
    got8, status8 = run_sim(sim, frames, present, cw, ch, w, h, desc(ow, oh, dtype=0, aa=aa), rois)
    for r, roi in enumerate(rois):
        st, box = ri.clip(roi, len(frames), w, h)
        if st and not present[roi[0]]:
            st = ri.EMPTY
        assert status[r] == status8[r] == st, (r, roi)
        if not st:
            assert not got[r].any() and not got8[r].any(), (r, roi)
            continue
        want = reference(src[roi[0]], size, box, bool(aa))
        check(got[r], want, torch.float32)
        check(got[r].to(torch.float16), want, torch.float16)
        check(got[r].to(torch.bfloat16), want, torch.bfloat16)
        if oh >= ri.U8_CHECK_SIZE[0] and ow >= ri.U8_CHECK_SIZE[1]:
            check(got8[r].to(torch.uint8), reference(src[roi[0]], size, box, bool(aa), u8=True), torch.uint8)
        if (box[3], box[2]) == (oh, ow):
            assert np.array_equal(got8[r].numpy().astype(np.int32), src[roi[0]][:, box[1]:box[1] + oh, box[0]:box[0] + ow]), "identity"


@pytest.mark.parametrize("aa", [1, 0], ids=["aa", "plain"])
@pytest.mark.parametrize("size", ri.SIZES, ids=["%dx%d" % (s[1], s[0]) for s in ri.SIZES])
def test_mixed_boxes_match_torch(sim, frames352, size, aa):
    frames, src = frames352
    check_rows(sim, frames, src, ri.W, ri.H, ri.W, ri.H, ri.MIXED, size, aa)


@pytest.mark.parametrize("size", ri.SIZES, ids=["%dx%d" % (s[1], s[0]) for s in ri.SIZES])
def test_bad_boxes_match_torch(sim, frames352, size):
    frames, src = frames352
    check_rows(sim, frames, src, ri.W, ri.H, ri.W, ri.H, ri.BAD, size, 1)


def test_cycle_boxes_match_torch(sim, frames352):
    frames, src = frames352
    check_rows(sim, frames, src, ri.W, ri.H, ri.W, ri.H, ri.CYCLE16, ri.CYCLE_SIZE, 1)


def test_absent_picture_gives_empty_rows(sim, frames352):
    frames, src = frames352
    check_rows(sim, frames, src, ri.W, ri.H, ri.W, ri.H, ri.MIXED, (48, 64), 1, present=[1, 0, 1])


@pytest.mark.parametrize("case", sorted(ri.MANY_TAPS))
def test_many_taps_match_torch(sim, case):
    fixture, box, size = ri.MANY_TAPS[case]
    w, h, cw, ch = (1920, 1080, 1920, 1088) if fixture == "cfg2_1080p" else (ri.W, ri.H, ri.W, ri.H)
    frames = random_frame(cw, ch, 31)[None]
    src = [rgb(*planes(frames[0], cw, ch), w, h)]
    for aa in (1, 0):
        got, status = run_sim(sim, frames, [1], cw, ch, w, h, desc(size[1], size[0], aa=aa), [(0,) + box])
        assert status.tolist() == [ri.INSIDE]
        check(got[0], reference(src[0], size, box, bool(aa)), torch.float32)


# ---------------------------------------------------------------------------------------------------- rois_from_xyxy

def test_rois_from_xyxy():
    from jsmpeg_amd import tensor
    boxes = torch.tensor([[10.0, 20.0, 30.0, 40.0], [10.2, 20.7, 30.1, 40.9], [-3.5, -0.5, 5.5, 7.0], [5.0, 5.0, 5.0, 5.0],
                          [9.0, 9.0, 3.0, 3.0], [float("nan"), 0.0, 5.0, 5.0], [-1e12, -1e12, 1e12, 1e12]])
    rows = torch.tensor([0, 2, 1, 0, 0, 1, 2])
    r = tensor.rois_from_xyxy(boxes, rows)
    assert r.dtype == torch.int32 and r.shape == (7, 5) and r.device == boxes.device
    assert r.tolist() == [[0, 10, 20, 20, 20], [2, 10, 20, 21, 21], [1, -4, -1, 10, 8], [0, 5, 5, 0, 0], [0, 9, 9, -6, -6],
                          [1, 0, 0, 0, 0], [2, ri.I32_MIN, ri.I32_MIN, ri.I32_MAX, ri.I32_MAX]]
    # the detector saw a 176 x 144 input of a 352 x 288 picture; two pixels of context on every side
    r = tensor.rois_from_xyxy(boxes[:2], rows[:2], scale=(2, 2), pad=2)
    assert r.tolist() == [[0, 18, 38, 44, 44], [2, 18, 39, 45, 45]]
    assert tensor.rois_from_xyxy(boxes[:2], rows[:2], scale=(2, 0.5)).tolist() == [[0, 20, 10, 40, 10], [2, 20, 10, 41, 11]]
    assert tensor.rois_from_xyxy(torch.zeros((0, 4)), torch.zeros((0,), dtype=torch.int64)).shape == (0, 5)
    for bad in ((torch.zeros((3, 5)), torch.zeros(3, dtype=torch.int32)), (torch.zeros((3, 4)), torch.zeros(2, dtype=torch.int32)),
                (torch.zeros((3, 4)), torch.zeros(3))):
        with pytest.raises(ValueError):
            tensor.rois_from_xyxy(*bad)


# ------------------------------------------------------------------------------------------- the library, the kernel

def test_library_exports_the_roi_calls():
    from jsmpeg_amd import build, tensor
    lib = ctypes.CDLL(build.LIB_HIP)
    for name in tensor.ROI_SYMBOLS:
        assert hasattr(lib, name), name


def test_roi_kernel_has_no_scratch_and_no_more_lds_than_k_tensor():
    from jsmpeg_amd import build
    usage = build.check_kernel_resources()
    roi = [n for n in usage if "k_tensor_roi" in n]
    base = [n for n in usage if "k_tensor" in n and "k_tensor_roi" not in n]
    assert len(roi) == 1 and len(base) == 1, sorted(usage)
    assert usage[roi[0]]["ScratchSize"] == 0, usage[roi[0]]
    assert 0 < usage[roi[0]]["LDS Size"] <= usage[base[0]]["LDS Size"], (usage[roi[0]], usage[base[0]])
