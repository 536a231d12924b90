"""NumPy restatement of run_eval's image summaries (tf_utils/common.py:118-168, tf_train.py:329-376) for arbitrary shapes: what
iaf_img_range / iaf_img_grid (include/iaf_hip.h) and EvalPass.images() are held to.  Pinned to the reference's own functions by
tests/golden/image_grids.npz (tests/test_images_reference.py).  TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np


def stretch(a):
    """img_stretch: fp32, shifted by the minimum and divided by (the maximum of the shifted array + 1e-12), over the WHOLE array"""
    a = np.array(a, dtype=np.float32)
    a = a - a.min()
    d = np.float32(np.float64(a.max()) + 1e-12)
    return (a / d).astype(np.float32)


def grid_shape(n, H, W, aspect_ratio=1.0):
    ar = aspect_ratio * (W / float(H))
    return int(math.ceil(math.sqrt(n * ar))), int(math.ceil(math.sqrt(n / ar)))


def tile(imgs, border=0, border_color=0.0, aspect_ratio=1.0):
    """img_tile of NHWC images: [(H + border) * th - border, (W + border) * tw - border, C], image i at tile (i // tw, i % tw)"""
    imgs = np.asarray(imgs)
    n, H, W, C = imgs.shape
    th, tw = grid_shape(n, H, W, aspect_ratio)
    out = np.full(((H + border) * th - border, (W + border) * tw - border, C), border_color, dtype=np.float32)
    for i in range(min(n, th * tw)):
        y, x = (H + border) * (i // tw), (W + border) * (i % tw)
        out[y:y + H, x:x + W] = imgs[i]
    return out


def grid(sources, n_imgs, border=0, border_color=0.0):
    """iaf_amd.images.image_grid's float grid: sources = [(NCHW array, stretch_over, then_over or None), ...]; slot s shows image
    s // len(sources) of source s % len(sources)"""
    ns = len(sources)
    shown = []
    for a, over, then in sources:
        a = np.asarray(a)
        if then is None:
            shown.append(stretch(a[:over]))
        else:
            shown.append(stretch(stretch(a[:over])[:then]))
    C, H, W = np.asarray(sources[0][0]).shape[1:]
    imgs = np.zeros((n_imgs, H, W, C), np.float32)
    for s in range(n_imgs):
        imgs[s] = np.transpose(shown[s % ns][s // ns], (1, 2, 0))
    return tile(imgs, border, border_color)


def quantise(grid_f32):
    """the package's byte rule (include/iaf_hip.h): floor(fp64(v) * 255 + 0.5) clamped to [0, 255], NaN -> 0"""
    q = np.floor(np.asarray(grid_f32, dtype=np.float64) * 255.0 + 0.5)
    q = np.where(np.isnan(q), 0.0, np.clip(q, 0.0, 255.0))
    return q.astype(np.uint8)
