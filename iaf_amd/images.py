"""run_eval's image summaries (tf_train.py:329-376): img_stretch and img_tile (tf_utils/common.py:118-168) for images that are already
on the device -- iaf_img_range and iaf_img_grid (include/iaf_hip.h has the arithmetic) -- and a PNG writer, so that the result is a file.

img_stretch shifts and scales by the minimum and maximum of the WHOLE array it is given; a source here names that array as a number of
leading rows (the reference's [:cur]), and run_eval's samples are stretched twice, over the batch and then over the rows shown."""
import math
import struct
import zlib

import torch

from . import _capi
from ._capi import ptr as _ptr, stream as _stream


def grid_shape(n, H, W, aspect_ratio=1.0):
    """(th, tw): the tiles of img_tile's grid for n images of H x W pixels (common.py:141-144)"""
    if not _capi.int_in(n, 1) or not _capi.int_in(H, 1) or not _capi.int_in(W, 1):
        raise ValueError("grid_shape: n, H and W must be positive ints, got %r, %r, %r" % (n, H, W))
    if isinstance(aspect_ratio, bool) or not isinstance(aspect_ratio, (int, float)) or not math.isfinite(aspect_ratio) or aspect_ratio <= 0:
        raise ValueError("grid_shape: aspect_ratio must be a positive finite number, got %r" % (aspect_ratio,))
    ar = aspect_ratio * (W / float(H))
    return int(math.ceil(math.sqrt(n * ar))), int(math.ceil(math.sqrt(n / ar)))


def _rows(v, t, what):
    if not _capi.int_in(v, 1, int(t.shape[0]) + 1):
        raise ValueError("image_grid: %s must be an int in [1, %d], got %r" % (what, int(t.shape[0]), v))
    return v


def image_grid(sources, n_imgs, border=0, border_color=0.0, u8=True, f32=True):
    """The grid of n_imgs tiles as device tensors [Hg, Wg, C]: (grid_u8 or None, grid_f32 or None, records).

    sources: 1 or 2 entries (tensor, stretch_over, then_over=None) -- a contiguous NCHW uint8 or fp32 device tensor with C = 1 or 3,
    stretched over its first stretch_over rows and then, when then_over is given (then_over <= stretch_over), over its first
    then_over rows of the result.  Slot s shows image s // len(sources) of source s % len(sources); the images shown must lie within
    the rows the last stretch ran over.  One iaf_img_range launch per record and one iaf_img_grid; no synchronisation, capturable.
    The 16-byte records come back as the third element: an int32 [n_records, 4] device tensor whose column 2 holds the counts of
    non-finite elements (a source with a count > 0 shows NaN / 0, include/iaf_hip.h)."""
    if not isinstance(sources, (list, tuple)) or not 1 <= len(sources) <= 2:
        raise ValueError("image_grid: sources must be a list of 1 or 2 (tensor, stretch_over[, then_over]) entries")
    if not _capi.int_in(n_imgs, 1):
        raise ValueError("image_grid: n_imgs must be a positive int, got %r" % (n_imgs,))
    if not _capi.int_in(border, 0):
        raise ValueError("image_grid: border must be a non-negative int, got %r" % (border,))
    if isinstance(border_color, bool) or not isinstance(border_color, (int, float)) or not math.isfinite(border_color):
        raise ValueError("image_grid: border_color must be a finite number, got %r" % (border_color,))
    if not isinstance(u8, bool) or not isinstance(f32, bool) or not (u8 or f32):
        raise ValueError("image_grid: u8 and f32 must be True or False, and not both False")
    ns = len(sources)
    parsed, shape, dev = [], None, None
    for s, entry in enumerate(sources):
        if not isinstance(entry, (list, tuple)) or not 2 <= len(entry) <= 3:
            raise ValueError("image_grid: sources[%d] must be (tensor, stretch_over[, then_over])" % s)
        t, over, then = entry[0], entry[1], (entry[2] if len(entry) == 3 else None)
        if not (torch.is_tensor(t) and t.dtype in (torch.uint8, torch.float32) and t.is_cuda and t.dim() == 4 and t.is_contiguous()
                and t.shape[1] in (1, 3) and min(t.shape) >= 1):
            raise ValueError("image_grid: sources[%d] must be a contiguous uint8 or fp32 [n,C,H,W] device tensor with C = 1 or 3" % s)
        if shape is None:
            shape, dev = tuple(int(v) for v in t.shape[1:]), t.device
        elif tuple(int(v) for v in t.shape[1:]) != shape or t.device != dev:
            raise ValueError("image_grid: the sources must share C, H, W and the device")
        _rows(over, t, "stretch_over")
        if then is not None and _rows(then, t, "then_over") > over:
            raise ValueError("image_grid: then_over (%d) must lie within stretch_over (%d)" % (then, over))
        shown = (n_imgs - s + ns - 1) // ns
        if shown > (over if then is None else then):
            raise ValueError("image_grid: %d images of sources[%d] are shown, its last stretch covers %d rows" % (shown, s, then or over))
        parsed.append((t, over, then))
    C, H, W = shape
    th, tw = grid_shape(n_imgs, H, W)
    Hg, Wg = (H + border) * th - border, (W + border) * tw - border
    lib, per = _capi.lib(), C * H * W
    with torch.cuda.device(dev):
        records = torch.zeros((sum(1 if then is None else 2 for _, _, then in parsed), 4), dtype=torch.int32, device=dev)
        table, r = (_capi.ImgSource * ns)(), 0
        for s, (t, over, then) in enumerate(parsed):
            dt = _capi.IAF_IMG_U8 if t.dtype == torch.uint8 else _capi.IAF_IMG_F32
            table[s].ptr, table[s].dtype = t.data_ptr(), dt
            for rows, field in ((over, "outer"), (then, "inner")):
                if rows is not None:
                    _capi.check(lib.iaf_img_range(_ptr(t), dt, rows * per, _ptr(records[r]), _stream()))
                    setattr(table[s], field, records[r].data_ptr())
                    r += 1
        g8 = torch.empty((Hg, Wg, C), dtype=torch.uint8, device=dev) if u8 else None
        gf = torch.empty((Hg, Wg, C), dtype=torch.float32, device=dev) if f32 else None
        _capi.check(lib.iaf_img_grid(table, ns, n_imgs, C, H, W, border, float(border_color), _ptr(gf), _ptr(g8), _stream()))
    torch.autograd.graph.increment_version((records,) + tuple(g for g in (g8, gf) if g is not None))      # (raw-pointer writes: tell torch)
    return g8, gf, records


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)


def write_png(path_or_file, grid_u8):
    """Write a [H, W], [H, W, 1] (greyscale) or [H, W, 3] (RGB) uint8 grid -- a host tensor or an ndarray -- as an 8-bit, non-interlaced
    PNG with filter type 0 on every row.  The standard library only; path_or_file: a path or an object with write()."""
    g = grid_u8
    if torch.is_tensor(g):
        if g.is_cuda:
            raise ValueError("write_png: a host tensor or ndarray (copy the grid with .cpu() first)")
        g = g.numpy()
    shape = tuple(int(v) for v in getattr(g, "shape", ()))
    if str(getattr(g, "dtype", "")) != "uint8" or len(shape) not in (2, 3) or min(shape, default=0) < 1 or (len(shape) == 3 and shape[2] not in (1, 3)):
        raise ValueError("write_png: a uint8 grid [H,W], [H,W,1] or [H,W,3] with at least one pixel, got %r" % (getattr(g, "shape", g),))
    H, W, C = shape[0], shape[1], (shape[2] if len(shape) == 3 else 1)
    rows = g.reshape(H, W * C)
    raw = b"".join(b"\x00" + rows[y].tobytes() for y in range(H))
    png = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2 if C == 3 else 0, 0, 0, 0))
           + _chunk(b"IDAT", zlib.compress(raw, 9)) + _chunk(b"IEND", b""))
    if hasattr(path_or_file, "write"):
        path_or_file.write(png)
    else:
        with open(path_or_file, "wb") as f:
            f.write(png)
