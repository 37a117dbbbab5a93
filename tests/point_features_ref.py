"""numpy restatement of votenet_subsample_augment_features (include/votenet_point_features.h, libvotenet_features.so): the points of votenet_subsample_augment (float64
transform in the reference's order, one rounding to float), the carried raw columns, and the height above the scene's floor -- the
rank formula of np.percentile(up, 0.99) with linear interpolation, in double, rounded once."""
import numpy as np


def points_ref(rows, depth_to_camera=True, flip=0, angle=0.0, scale=1.0, train=False, cos_sin=None):
    """rows (n, >= 3) raw rows already picked -> (n, 3) float32: augment.hip's arithmetic (dataset.py:302-308, sunutils.py:70-77,133-139)."""
    p = np.asarray(rows, dtype=np.float64)
    x, y, z = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()
    if depth_to_camera:
        y, z = -z, y
    if train:
        if flip & 1:
            x = -x
        if flip & 2:
            z = -z
        c, s = cos_sin if cos_sin is not None else (np.cos(angle), np.sin(angle))  # (cos_sin: the values the entry was given)
        xr = c * x + s * z
        zr = -s * x + c * z
        x, y, z = xr * scale, y * scale, zr * scale
    return np.stack([x, y, z], 1).astype(np.float32)


def floor_ref(up):
    """up: float32 values of one scene -> (floor float32, a, b float32 order statistics, m): the finite values only; k = 0.0099 (m - 1),
    lo = floor(k), t = k - lo, a / b of rank lo / min(lo + 1, m - 1), floor = float32(a + (b - a) t) in double.  m = 0: all zero."""
    up = np.asarray(up, dtype=np.float32)
    fin = np.sort(up[np.isfinite(up)])
    m = len(fin)
    if m == 0:
        return np.float32(0.0), np.float32(0.0), np.float32(0.0), 0
    k = 0.0099 * (m - 1)
    lo = int(np.floor(k))
    t = k - lo
    a, b = fin[lo], fin[min(lo + 1, m - 1)]
    return np.float32(np.float64(a) + (np.float64(b) - np.float64(a)) * t), a, b, m


def heights_ref(points, floor=None):
    """points (n, 3) float32 of one scene -> (n,) float32: up - floor in float32 (up = -y), 0 where up is not finite.  floor: the value to
    subtract (None: floor_ref's)."""
    up = -np.asarray(points, dtype=np.float32)[:, 1]
    fl = np.float32(floor_ref(up)[0] if floor is None else floor)
    with np.errstate(invalid="ignore"):
        h = (up - fl).astype(np.float32)
    h[~np.isfinite(up)] = 0.0
    return h


def ulp32(v):
    """The spacing of float32 at |v| (the bar of 'within one float32 ulp')."""
    return float(np.spacing(np.float32(abs(float(v)))))
