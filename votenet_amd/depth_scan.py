"""The raw scan from the depth image, on the device (libvotenet_depth.so, include/votenet_depth_scan.h).

The reference reads a scene's scan from a text file (np.loadtxt('depth/%06d.txt'), sunutils.py:178-180) that an offline pass over
SUN RGB-D's depth images wrote.  Here the dataset as it is distributed -- 16-bit depth PNG, colour image, Rtilt, K -- is enough:
scan_from_depth turns a batch of depth images into the `raw` / `raw_offset` that input_pipeline.subsample_augment,
subsample_augment_features, select_boxes and build_batch take, with the reference's own geometry
(SUNRGBD_Calibration.project_image_to_camera -> flip_axis_to_depth -> Rtilt, sunutils.py:107-121).  The rule is stated once, in the
header; tests/depth_scan_ref.py restates it in numpy.  Reading image files is the host's work: load_depth_png is the one helper."""
import ctypes

import numpy as np
import torch

from . import _lib as L
from . import input_pipeline as IP

ENCODINGS = {"sunrgbd": 0, "mm": 1}  # the dataset's PNGs hold the millimetres rotated left by three bits; "mm": plain millimetres
MAX_SCENES = 32      # per call: the calibrations travel as kernel arguments
TILE_PIXELS = 2048   # one workgroup's pixels (tests: the sizes either side of a tile)
PAPER_MAX_DEPTH = 8.0  # the dataset toolbox's clamp, metres


def load_depth_png(path):
    """A 16-bit depth PNG -> (h, w) uint16 array, the pixel values as stored (encoding "sunrgbd" for the dataset's files)."""
    from PIL import Image  # only here: nothing else in this module needs it
    with Image.open(path) as im:
        a = np.asarray(im)
    if a.ndim != 2 or a.dtype.kind not in "ui" or a.min() < 0 or a.max() > 0xffff:
        raise L.InvalidArgumentError("load_depth_png: %s is not a single-channel 16-bit image (shape %s, %s)" % (path, a.shape, a.dtype))
    return np.ascontiguousarray(a.astype(np.uint16))


def _flat(images, dtype, tdtype, tail, dev, what):
    """list of (h, w) + tail arrays / device tensors of `dtype` -> (one flat device tensor of their pixels, [(h, w)])."""
    flat, hw = [], []
    for i, im in enumerate(images):
        if torch.is_tensor(im):
            ok, shape = im.dtype == tdtype, tuple(im.shape)
        else:
            im = np.asarray(im)
            ok, shape = im.dtype == dtype, im.shape
        if not ok or len(shape) != 2 + len(tail) or tuple(shape[2:]) != tail or shape[0] < 1 or shape[1] < 1:
            raise L.InvalidArgumentError("scan_from_depth: %s[%d] must be (h, w%s) %s, got %s %s"
                                         % (what, i, "".join(", %d" % t for t in tail), np.dtype(dtype).name, tuple(shape), im.dtype))
        hw.append((int(shape[0]), int(shape[1])))
        flat.append(im)
    if all(not torch.is_tensor(f) for f in flat):  # the usual case: one upload
        host = np.ascontiguousarray(np.concatenate([f.reshape(-1) for f in flat]))
        return torch.from_numpy(host.view(np.int16) if dtype == np.uint16 else host).to(dev), hw
    parts = []
    for f in flat:
        if torch.is_tensor(f):
            f = f.contiguous().view(torch.int16) if tdtype == torch.uint16 else f.contiguous()
        else:
            f = np.ascontiguousarray(f)
            f = torch.from_numpy(f.view(np.int16) if dtype == np.uint16 else f)
        parts.append(f.reshape(-1).to(dev))
    return torch.cat(parts), hw


def scan_from_depth(depth, calib, rgb=None, encoding="sunrgbd", pixel_origin=1.0, max_depth=PAPER_MAX_DEPTH, capacity_rows=None):
    """depth: list of b (h, w) uint16 arrays or device tensors, sizes may differ from scene to scene.  calib: as for select_boxes,
    (Rtilt (b,3,3), K (b,3,3)) or a list of (Rtilt, K) pairs (sunrgbd.parse_calib).  rgb: None, or a list of (h, w, 3) uint8.
    encoding "sunrgbd" (the dataset's PNGs) or "mm"; pixel_origin 1.0: the 1-based pixel convention of the label files' box2d and K;
    max_depth: metres, deeper pixels are kept at max_depth.  A pixel of value 0 has no point.
    -> (raw (sum n_s, 3 or 6) float32 on the device, upright-depth coordinates [+ colour / 255], the valid pixels of each scene in
    row-major order; raw_offset host int64 (b+1), the one read-back).  capacity_rows: rows to allocate instead of one per pixel;
    more valid pixels than that raise."""
    if not isinstance(depth, (list, tuple)) or len(depth) < 1:
        raise L.InvalidArgumentError("scan_from_depth: depth must be a list of (h, w) uint16 images, one per scene")
    b = len(depth)
    if b > MAX_SCENES:
        raise L.InvalidArgumentError("scan_from_depth: at most %d scenes per call, got %d" % (MAX_SCENES, b))
    if encoding not in ENCODINGS:
        raise L.InvalidArgumentError("scan_from_depth: encoding must be one of %s, got %r" % (sorted(ENCODINGS), encoding))
    tensors = [t for t in list(depth) + list(rgb or []) if torch.is_tensor(t)]
    if any(not t.is_cuda for t in tensors):
        raise L.VotenetError("scan_from_depth: image tensors must live on the GPU (or be numpy arrays)")
    dev = tensors[0].device if tensors else torch.device("cuda", torch.cuda.current_device())
    if any(t.device != dev for t in tensors):
        raise L.InvalidArgumentError("scan_from_depth: the images live on different devices")
    d, hw = _flat(depth, np.uint16, torch.uint16, (), dev, "depth")
    c = None
    if rgb is not None:
        if not isinstance(rgb, (list, tuple)) or len(rgb) != b:
            raise L.InvalidArgumentError("scan_from_depth: %d depth images but %s colour images" % (b, len(rgb) if isinstance(rgb, (list, tuple)) else "no list of"))
        c, chw = _flat(rgb, np.uint8, torch.uint8, (3,), dev, "rgb")
        if chw != hw:
            raise L.InvalidArgumentError("scan_from_depth: depth images are %s, colour images %s" % (hw, chw))
    rt, km = IP._calib_arrays(calib, b, "scan_from_depth")
    hw = np.ascontiguousarray(hw, dtype=np.int32)
    off = np.zeros(b + 1, np.int64)
    off[1:] = np.cumsum(hw[:, 0].astype(np.int64) * hw[:, 1])
    total, stride = int(off[-1]), 3 if c is None else 6
    cap = total if capacity_rows is None else int(capacity_rows)
    if cap < 0:
        raise L.InvalidArgumentError("scan_from_depth: capacity_rows must be >= 0, got %d" % cap)
    D = L.side_lib("depth")
    raw = torch.empty((cap, stride), dtype=torch.float32, device=dev)
    off_dev = torch.empty((b + 1,), dtype=torch.int64, device=dev)
    wsb = int(D.votenet_depth_scan_workspace_bytes(b, total))
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    with L.device_guard(dev):
        L.check(D.votenet_depth_scan(b, L.ptr(d), L.ptr(c), IP._hp(off), hw.ctypes.data_as(ctypes.c_void_p), IP._hp(rt), IP._hp(km),
                                     ENCODINGS[encoding], float(pixel_origin), float(max_depth), L.ptr(raw), stride, cap, L.ptr(off_dev),
                                     L.ptr(ws), wsb, L.stream_ptr()), side="depth")
    raw_offset = off_dev.cpu().numpy()  # the one read-back (it also keeps d, c and ws alive until the kernels are through)
    if raw_offset[-1] > cap:
        raise L.InvalidArgumentError("scan_from_depth: %d valid pixels, capacity_rows = %d" % (int(raw_offset[-1]), cap))
    return raw[:int(raw_offset[-1])], raw_offset


def build_batch_from_depth(depth, calib, objects, rgb=None, encoding="sunrgbd", pixel_origin=1.0, max_depth=PAPER_MAX_DEPTH,
                           **build_batch_kwargs):
    """scan_from_depth, then input_pipeline.build_batch on its raw / raw_offset with the same calib and objects (aug, choice, seed,
    scene0, n_out, height, extra_cols: build_batch's).  With rgb, extra_cols=3 carries the colour to sa1.  A scene with fewer than
    n_out valid pixels is select_boxes' error.  -> build_batch's (points, gt, scene_index)."""
    raw, raw_offset = scan_from_depth(depth, calib, rgb, encoding, pixel_origin, max_depth)
    return IP.build_batch(raw, raw_offset, calib, objects, **build_batch_kwargs)
