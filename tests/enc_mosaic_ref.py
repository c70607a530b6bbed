"""TEST INFRASTRUCTURE ONLY -- the numpy restatement of the encoder's mosaic input (jsmpeg_amd/csrc/enc_mosaic.h), written from
the rule's text and sharing nothing with the header: every plane filled, enc_scale_ref.scaled_planes of each cell pasted in
index order, the edge replication."""
import numpy as np

import enc_scale_ref as es


def compose(cells, frames, width, height, fill=(16, 128, 128)):
    """cells: [(source w, source h, crop or None, antialias, x, y, w, h)]; frames: one source frame (Y | Cr | Cb of the source's
    coded size) or None per cell -> the encoder's frame Y | Cr | Cb of the coded size of width x height, uint8"""
    assert 1 <= len(cells) <= 64 and len(frames) == len(cells)
    cw, ch = es.coded(width, height)
    hw, hh = (width + 1) >> 1, (height + 1) >> 1
    planes = [np.full((height, width), fill[0], np.int64), np.full((hh, hw), fill[1], np.int64), np.full((hh, hw), fill[2], np.int64)]
    for (sw, sh, crop, aa, x, y, w, h), f in zip(cells, frames):
        assert x % 2 == 0 and y % 2 == 0 and w >= 1 and h >= 1 and x + w <= width and y + h <= height
        if f is None:
            continue
        for p, s, (px, py) in zip(planes, es.scaled_planes(f, sw, sh, w, h, crop, bool(aa)), ((x, y), (x >> 1, y >> 1), (x >> 1, y >> 1))):
            p[py:py + s.shape[0], px:px + s.shape[1]] = s
    ext = lambda p, w, h: np.pad(p, ((0, h - p.shape[0]), (0, w - p.shape[1])), mode="edge")
    return np.concatenate([ext(planes[0], cw, ch).ravel(), ext(planes[1], cw // 2, ch // 2).ravel(), ext(planes[2], cw // 2, ch // 2).ravel()]).astype(np.uint8)
