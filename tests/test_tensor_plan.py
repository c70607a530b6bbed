"""Part 7 (pictures as resized RGB tensors) without a GPU: tensor_plan.h -- the taps, the colour and the descriptor check
that k_tensor (kernels.hip) runs -- compiled by g++ into a TEST-ONLY simulator (tests/sim/sim_tensor.cpp) and held against
torch's CPU F.interpolate at the GPU tests' tolerances; the library's exports and the kernel's resources."""
import ctypes
import glob
import os
import subprocess
import zlib

import numpy as np
import pytest
import torch

from conftest import ROOT
from tensor_ref import IMAGENET_MEAN, IMAGENET_STD, check, planes, reference, rgb

CSRC = os.path.join(ROOT, "jsmpeg_amd", "csrc")


class Desc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("width", "height", "crop_x", "crop_y", "crop_width", "crop_height",
                                                "dtype", "layout", "order", "antialias")] + \
               [("mean", ctypes.c_float * 3), ("std", ctypes.c_float * 3)]


def desc(ow, oh, crop=(0, 0, 0, 0), dtype=3, layout=0, order=0, aa=1, mean=(0, 0, 0), std=(1, 1, 1)):
    return Desc(ow, oh, *crop, dtype, layout, order, aa, (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std))


@pytest.fixture(scope="module")
def sim():
    so = os.path.join(ROOT, "tests", "sim", "libjsmpeg_sim_tensor.so")
    src = os.path.join(ROOT, "tests", "sim", "sim_tensor.cpp")
    deps = [src] + glob.glob(os.path.join(CSRC, "*.h")) + [os.path.join(ROOT, "include", "jsmpeg_hip.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-I", CSRC,
                               "-I", os.path.join(ROOT, "include"), "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    lib.sim_tensor.restype = ctypes.c_int
    lib.sim_tensor.argtypes = [vp, u32, u32, u32, u32, ctypes.POINTER(Desc), vp]
    lib.sim_tensor_check.restype = ctypes.c_char_p
    lib.sim_tensor_check.argtypes = [ctypes.POINTER(Desc), u32, u32]
    lib.sim_bf16.restype = ctypes.c_uint16
    lib.sim_bf16.argtypes = [ctypes.c_float]
    return lib


def run_sim(sim, frame, cw, ch, w, h, d):
    out = np.zeros((3, d.height, d.width), dtype=np.float32)
    assert sim.sim_tensor(frame.ctypes.data, cw, ch, w, h, ctypes.byref(d), out.ctypes.data) == 0
    return torch.from_numpy(out)


def random_frame(cw, ch, seed):
    return np.random.default_rng(seed).integers(0, 256, cw * ch * 3 // 2, dtype=np.uint8)


# (display w, h, coded w, h, out (h, w) or None = identity, crop or None)
CASES = {
    "identity_1080p": (1920, 1080, 1920, 1088, None, None),
    "1080p_to_224": (1920, 1080, 1920, 1088, (224, 224), None),
    "1080p_to_320x180": (1920, 1080, 1920, 1088, (180, 320), None),
    "1080p_to_1000x563": (1920, 1080, 1920, 1088, (563, 1000), None),
    "upscale_2x_352x288": (352, 288, 352, 288, (576, 704), None),
    "to_1x1": (1920, 1080, 1920, 1088, (1, 1), None),
    "to_1x7": (352, 288, 352, 288, (1, 7), None),
    "to_7x1": (352, 288, 352, 288, (7, 1), None),
    "crop_odd_origin": (1920, 1080, 1920, 1088, (224, 224), (333, 101, 777, 555)),
    "crop_identity": (352, 288, 352, 288, None, (7, 3, 101, 57)),
    "odd_17x33_identity": (17, 33, 32, 48, None, None),
    "odd_17x33_to_5x9": (17, 33, 32, 48, (9, 5), None),
}


@pytest.mark.parametrize("aa", [1, 0], ids=["aa", "plain"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_simulator_matches_torch(sim, case, aa):
    w, h, cw, ch, size, crop = CASES[case]
    frame = random_frame(cw, ch, zlib.crc32(case.encode()))
    src = rgb(*planes(frame, cw, ch), w, h)
    oh, ow = size if size else ((crop[3], crop[2]) if crop else (h, w))
    c = crop or (0, 0, 0, 0)
    # f32, values in [0, 1]; f16 / bf16 are that value cast (the kernel's cast: round to nearest even)
    got = run_sim(sim, frame, cw, ch, w, h, desc(ow, oh, c, aa=aa))
    want = reference(src, (oh, ow), crop, bool(aa))
    check(got, want, torch.float32)
    check(got.to(torch.float16), want, torch.float16)
    bf = np.vectorize(lambda v: sim.sim_bf16(float(v)), otypes=[np.uint16])(got.numpy()[:, :8, :8])
    assert np.array_equal(bf.view(np.int16), got[:, :8, :8].to(torch.bfloat16).view(torch.int16).numpy())
    # ImageNet normalisation, BGR
    got = run_sim(sim, frame, cw, ch, w, h, desc(ow, oh, c, aa=aa, order=1, mean=IMAGENET_MEAN[::-1], std=IMAGENET_STD[::-1]))
    check(got, reference(src, (oh, ow), crop, bool(aa), "bgr", IMAGENET_MEAN[::-1], IMAGENET_STD[::-1]), torch.float32)
    # u8
    got = run_sim(sim, frame, cw, ch, w, h, desc(ow, oh, c, dtype=0, aa=aa))
    want = reference(src, (oh, ow), crop, bool(aa), u8=True)
    check(got.to(torch.uint8), want, torch.uint8)
    if size is None:
        assert torch.equal(got, want), "u8 at identity size must be bit-exact"


def test_identity_even_width_is_read_rgba(sim):
    """even widths: the identity tensor is read_rgba's RGB (the renderer's formula, the reference's running indices)"""
    w, h, cw, ch = 352, 288, 352, 288
    frame = random_frame(cw, ch, 7)
    y, cr, cb = planes(frame, cw, ch)
    got = run_sim(sim, frame, cw, ch, w, h, desc(w, h, dtype=0)).numpy().astype(np.int32)
    rgba = np.empty((h, w, 3), np.int32)      # canvas2d.js:64-119 for an even width: two rows per chroma row, two columns per chroma column
    for r in range(h):
        for x in range(w):
            Y, CR, CB = int(y[r, x]), int(cr[r >> 1, x >> 1]), int(cb[r >> 1, x >> 1])
            rr = (CR + ((CR * 103) >> 8)) - 179
            gg = ((CB * 88) >> 8) - 44 + ((CR * 183) >> 8) - 91
            bb = (CB + ((CB * 198) >> 8)) - 227
            rgba[r, x] = (min(max(Y + rr, 0), 255), min(max(Y - gg, 0), 255), min(max(Y + bb, 0), 255))
    assert np.array_equal(got.transpose(1, 2, 0), rgba)


@pytest.mark.parametrize("bad,why", [
    (dict(crop=(1900, 0, 100, 100)), "crop"),
    (dict(crop=(0, 1000, 100, 100)), "crop"),
    (dict(crop=(0, 0, 100, 0)), "crop"),
    (dict(crop=(5, 5, 0, 0)), "crop"),
    (dict(ow=0), "width"),
    (dict(oh=0), "width"),
    (dict(ow=4097), "width"),
    (dict(oh=4097), "width"),
    (dict(dtype=4), "dtype"),
    (dict(layout=2), "layout"),
    (dict(order=2), "order"),
    (dict(aa=2), "antialias"),
    (dict(std=(1, 0, 1)), "std"),
    (dict(std=(1, 1, float("nan"))), "finite"),
    (dict(mean=(float("inf"), 0, 0)), "finite"),
])
def test_descriptor_check_rejects(sim, bad, why):
    kw = dict(ow=224, oh=224)
    kw.update(bad)
    msg = sim.sim_tensor_check(ctypes.byref(desc(**kw)), 1920, 1080).decode()
    assert why in msg, msg
    out = np.zeros((3, 1, 1), np.float32)
    assert sim.sim_tensor(random_frame(1920, 1088, 1).ctypes.data, 1920, 1088, 1920, 1080, ctypes.byref(desc(**kw)), out.ctypes.data) == -1


def test_descriptor_check_accepts(sim):
    for kw in (dict(ow=4096, oh=1), dict(ow=1, oh=4096), dict(ow=8, oh=8, crop=(1919, 1079, 1, 1)), dict(ow=8, oh=8, dtype=0, std=(0, 0, 0))):
        kw2 = dict(kw)
        assert sim.sim_tensor_check(ctypes.byref(desc(kw2.pop("ow"), kw2.pop("oh"), **kw2)), 1920, 1080).decode() == ""


def test_library_exports_part7():
    from jsmpeg_amd import build, tensor
    lib = ctypes.CDLL(build.LIB_HIP)
    for name in tensor.SYMBOLS:
        assert hasattr(lib, name), name


def test_tensor_kernel_has_no_scratch():
    from jsmpeg_amd import build
    usage = build.check_kernel_resources()
    k = [n for n in usage if "k_tensor" in n]
    assert k, sorted(usage)
    for n in k:
        assert usage[n]["ScratchSize"] == 0, (n, usage[n])
        assert usage[n].get("LDS Size", 0) <= 64 * 1024, (n, usage[n])


def test_python_module_imports_without_a_gpu():
    from jsmpeg_amd import batch, live, tensor  # noqa: F401
    assert ctypes.sizeof(tensor.TensorDesc) == ctypes.sizeof(Desc) == 64
