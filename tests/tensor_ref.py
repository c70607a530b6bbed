"""The value a part-7 tensor must hold (include/jsmpeg_hip.h part 7), restated on the host for the tests: the integer
RGB in numpy, the resize and normalisation by torch on the CPU, and the tolerances per dtype."""
import numpy as np
import torch
import torch.nn.functional as F

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
DTYPES = {"u8": torch.uint8, "f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


def planes(frame, cw, ch):
    """Y | Cr | Cb bytes of one coded frame -> (Y [ch][cw], Cr, Cb [ch/2][cw/2])"""
    frame = np.asarray(frame, dtype=np.uint8).reshape(-1)
    y = frame[:cw * ch].reshape(ch, cw)
    cr = frame[cw * ch:cw * ch * 5 // 4].reshape(ch // 2, cw // 2)
    cb = frame[cw * ch * 5 // 4:cw * ch * 3 // 2].reshape(ch // 2, cw // 2)
    return y, cr, cb


def rgb(y, cr, cb, w, h):
    """display pixels (x, y) -> the Canvas2D integer BT.601, [3][h][w] int32, unsheared for any width"""
    ry, rx = np.arange(h) >> 1, np.arange(w) >> 1
    Y = y[:h, :w].astype(np.int32)
    CR = cr[ry][:, rx].astype(np.int32)
    CB = cb[ry][:, rx].astype(np.int32)
    r = (CR + ((CR * 103) >> 8)) - 179
    g = ((CB * 88) >> 8) - 44 + ((CR * 183) >> 8) - 91
    b = (CB + ((CB * 198) >> 8)) - 227
    return np.clip(np.stack([Y + r, Y - g, Y + b]), 0, 255).astype(np.int32)


def reference(rgb_chw, size=None, crop=None, antialias=True, order="rgb", mean=None, std=None, u8=False):
    """[3][h][w] integer RGB of one picture -> the float32 value of the tensor row in NCHW and the tensor's channel order
    (u8: the rounded, clamped value)"""
    x = torch.from_numpy(np.ascontiguousarray(rgb_chw)).float()
    if crop is not None and crop[2] and crop[3]:
        cx, cy, cw, ch = crop
        x = x[:, cy:cy + ch, cx:cx + cw]
    oh, ow = size if size is not None else x.shape[1:]
    if ow == 1 and antialias and oh != x.shape[1]:
        # torch's 2-D antialiased CPU kernel gets the vertical pass over a ONE-column intermediate wrong (tens of levels off,
        # while the same pass over a wider image is right): the same two passes, the vertical one run as a horizontal one
        h = F.interpolate(x[None], size=(x.shape[1], 1), mode="bilinear", align_corners=False, antialias=True)
        v = F.interpolate(h.transpose(-1, -2), size=(1, oh), mode="bilinear", align_corners=False, antialias=True).transpose(-1, -2)[0]
    else:
        v = F.interpolate(x[None], size=(oh, ow), mode="bilinear", align_corners=False, antialias=antialias)[0]
    if order == "bgr":
        v = v.flip(0)
    if u8:
        return torch.round(v).clamp(0, 255)
    m = torch.tensor(mean if mean is not None else (0.0, 0.0, 0.0), dtype=torch.float32)[:, None, None]
    s = torch.tensor(std if std is not None else (1.0, 1.0, 1.0), dtype=torch.float32)[:, None, None]
    return (v / 255 - m) / s


def _ordered(bits):
    b = bits.astype(np.int64) & 0xffff
    return np.where(b & 0x8000, -(b & 0x7fff), b)


def check(got, want, dtype):
    """got: the tensor row (torch, CPU) in NCHW; want: reference()'s float32 value.  Raises AssertionError with the worst place."""
    got = got.cpu()
    if dtype == torch.float32:
        d = (got - want).abs()
        assert float(d.max()) <= 5e-5, "f32: max error %g at %s" % (float(d.max()), np.unravel_index(int(d.argmax()), d.shape))
    elif dtype in (torch.float16, torch.bfloat16):
        # the f32 value cast, or one ulp from it -- or, where normalisation cancels to almost 0 and an ulp of the narrow
        # type is far below the f32 tolerance, within that tolerance
        w = want.to(dtype)
        d = np.abs(_ordered(got.view(torch.int16).numpy()) - _ordered(w.view(torch.int16).numpy()))
        d[(got.float() - want).abs().numpy() <= 5e-5] = 0
        assert d.max() <= 1, "%s: %d ulp at %s (got %r, want %r)" % (dtype, d.max(), np.unravel_index(int(d.argmax()), d.shape),
                                                                   float(got.flatten()[int(d.argmax())]), float(want.flatten()[int(d.argmax())]))
    else:
        d = (got.to(torch.int32) - want.to(torch.int32)).abs()
        assert int(d.max()) <= 1, "u8: off by %d at %s" % (int(d.max()), np.unravel_index(int(d.argmax()), d.shape))
        exact = float((d == 0).float().mean())
        assert exact >= 0.999, "u8: only %.4f%% exact" % (100 * exact)
