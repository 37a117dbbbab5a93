"""Host restatement (numpy float64, operation for operation) of include/votenet_depth_scan.h: the raw scan of a scene from its depth
image.  Every product, sum and quotient below is one float64 operation in the header's order (numpy does not fuse them) and every
output is rounded once to float32, so the rows equal the device's bit for bit."""
import numpy as np

ENCODINGS = {"sunrgbd": 0, "mm": 1}


def decode(p, encoding):
    """uint16 pixel values -> uint16 millimetres.  0 / "sunrgbd": the dataset's PNGs, rotated right by three bits; 1 / "mm": as stored."""
    p = np.asarray(p, np.uint16)
    enc = ENCODINGS.get(encoding, encoding)
    if enc == 0:
        q = p.astype(np.uint32)
        return (((q >> 3) | (q << 13)) & 0xffff).astype(np.uint16)
    if enc == 1:
        return p.copy()
    raise ValueError("unknown encoding %r" % (encoding,))


def metres(d16, max_depth=8.0):
    z = d16.astype(np.float64) / 1000.0
    return np.where(z > max_depth, np.float64(max_depth), z)


def scan_one(depth, rtilt, k, rgb=None, encoding=0, pixel_origin=1.0, max_depth=8.0):
    """(h, w) uint16, Rtilt (3, 3), K (3, 3) [, (h, w, 3) uint8] -> (n_valid, 3 or 6) float32, row-major pixel order."""
    depth = np.asarray(depth)
    assert depth.dtype == np.uint16 and depth.ndim == 2
    R, K = np.asarray(rtilt, np.float64).reshape(3, 3), np.asarray(k, np.float64).reshape(3, 3)
    d16 = decode(depth, encoding)
    row, col = np.nonzero(d16 != 0)  # row-major
    z = metres(d16[row, col], max_depth)
    u = col.astype(np.float64) + np.float64(pixel_origin)
    v = row.astype(np.float64) + np.float64(pixel_origin)
    x = ((u - K[0, 2]) * z) / K[0, 0]
    y = ((v - K[1, 2]) * z) / K[1, 1]
    p = (x, z, -y)
    out = [((R[i, 0] * p[0] + R[i, 1] * p[1]) + R[i, 2] * p[2]).astype(np.float32) for i in range(3)]
    if rgb is not None:
        rgb = np.asarray(rgb)
        assert rgb.dtype == np.uint8 and rgb.shape == depth.shape + (3,)
        c = (rgb[row, col].astype(np.float64) / 255.0).astype(np.float32)
        out += [c[:, 0], c[:, 1], c[:, 2]]
    return np.ascontiguousarray(np.stack(out, 1)) if len(row) else np.zeros((0, len(out)), np.float32)


def scan(depth, calib, rgb=None, encoding=0, pixel_origin=1.0, max_depth=8.0):
    """Lists of per-scene images and (Rtilt, K) pairs -> (raw (sum n_s, stride) float32, raw_offset int64 (b+1))."""
    rows = [scan_one(d, c[0], c[1], None if rgb is None else rgb[i], encoding, pixel_origin, max_depth)
            for i, (d, c) in enumerate(zip(depth, calib))]
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    return np.ascontiguousarray(np.concatenate(rows, 0)), off


def project_upright_depth_to_image(pc, rtilt, k):
    """sunutils.py:85-99 restated: (n, 3) upright-depth points -> (uv (n, 2), depth (n))."""
    R, K = np.asarray(rtilt, np.float64).reshape(3, 3), np.asarray(k, np.float64).reshape(3, 3)
    pc2 = np.dot(np.transpose(R), np.transpose(np.asarray(pc, np.float64)[:, 0:3]))
    cam = np.transpose(pc2).copy()
    cam[:, [0, 1, 2]] = cam[:, [0, 2, 1]]
    cam[:, 1] *= -1
    uv = np.dot(cam, np.transpose(K))
    uv[:, 0] /= uv[:, 2]
    uv[:, 1] /= uv[:, 2]
    return uv[:, 0:2], cam[:, 2]


# ---- inputs the CPU and GPU tests share ----
def tilted_calib(rng, h, w):
    """A calibration like the dataset's: a rotation a few degrees about x and z, focal length about the image's width."""
    a, c = rng.uniform(-0.3, 0.3), rng.uniform(-0.1, 0.1)
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    f = w * rng.uniform(0.7, 0.9)
    K = np.array([[f, 0, w / 2 + rng.uniform(-3, 3)], [0, f * rng.uniform(0.98, 1.02), h / 2 + rng.uniform(-3, 3)], [0, 0, 1]])
    return np.ascontiguousarray(rz @ rx), K


def encode(mm, encoding):
    """uint16 millimetres -> the pixel values that decode() turns back into them."""
    mm = np.asarray(mm, np.uint16).astype(np.uint32)
    return (((mm << 3) | (mm >> 13)) & 0xffff).astype(np.uint16) if ENCODINGS.get(encoding, encoding) == 0 else mm.astype(np.uint16)


def random_depth(rng, h, w, encoding=0, zeros=0.3, lo=400, hi=9500):
    """(h, w) uint16 pixel values: millimetres in [lo, hi) (some beyond the 8 m clamp), a share `zeros` of them 0."""
    mm = rng.integers(lo, hi, (h, w)).astype(np.uint16)
    mm[rng.random((h, w)) < zeros] = 0
    return encode(mm, encoding)
