"""Generate tests/golden/depth_scan.npz.

Runs where the reference tree is mounted:

    python tests/golden/make_depth_scan_golden.py <reference tree>      (or VOTENET_REFERENCE=<reference tree>)

The expected points come from the reference's own code, imported and called as make_box_points_golden.py does: a calibration file is
written to a temporary directory for sunutils.SUNRGBD_Calibration, and the valid pixels of a 53 x 61 synthetic depth image go through
its project_image_to_camera -> flip_axis_to_depth -> np.dot(Rtilt, .) (sunutils.py:107-121, the chain of
project_image_to_upright_camerea before its last flip).  cv2, which sunutils imports and these functions never use, is an empty
stand-in module.  The image holds random 16-bit values in the dataset's encoding (millimetres rotated left by three bits; 0.4 to 9.5 m,
so some lie beyond the toolbox's 8 m clamp), 30 % of them zero; Rtilt is tilted about two axes.  (u, v) are the 1-based pixel
coordinates in which the dataset's K and label files are written.  Only data is written: the image, the calibration's two lines of
text and matrices, and the reference's float64 points in row-major pixel order.
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ["VOTENET_REFERENCE"]
sys.modules.setdefault("cv2", types.ModuleType("cv2"))
sys.path.insert(0, REF)
import sunutils as SU  # noqa: E402

H, W = 53, 61
MAX_DEPTH = 8.0  # metres: the dataset toolbox's clamp


def main():
    rng = np.random.default_rng(20241019)
    a, c = 0.21, -0.07  # radians about x and about z
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    rtilt = rz @ rx
    k = np.array([[47.318, 0, 31.27], [0, 47.902, 26.81], [0, 0, 1]])
    text = " ".join(repr(float(x)) for x in rtilt.reshape(-1, order="F")) + "\n" + " ".join(repr(float(x)) for x in k.reshape(-1, order="F")) + "\n"
    mm = rng.integers(400, 9500, (H, W)).astype(np.uint32)
    mm[rng.random((H, W)) < 0.3] = 0
    image = (((mm << 3) | (mm >> 13)) & 0xffff).astype(np.uint16)  # what the dataset's PNG holds
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "calib.txt")
        with open(path, "w") as f:
            f.write(text)
        calib = SU.SUNRGBD_Calibration(path)
    assert np.array_equal(calib.Rtilt, rtilt) and np.array_equal(calib.K, k)
    row, col = np.nonzero(mm != 0)
    z = np.minimum(mm[row, col] / 1000.0, MAX_DEPTH)
    uv_depth = np.stack([col + 1.0, row + 1.0, z], 1)
    cam = calib.project_image_to_camera(uv_depth)
    points = np.transpose(np.dot(calib.Rtilt, np.transpose(calib.flip_axis_to_depth(cam))))
    print("%d x %d pixels, %d valid, %d clamped at %g m, |coordinate| <= %.3f" % (H, W, len(row), int((mm[row, col] > 1000 * MAX_DEPTH).sum()),
                                                                              MAX_DEPTH, np.abs(points).max()))
    out = os.path.join(HERE, "depth_scan.npz")
    np.savez_compressed(out, image=image, rtilt=np.ascontiguousarray(calib.Rtilt), k=np.ascontiguousarray(calib.K),
                        calib_text=np.array(text), points=np.ascontiguousarray(points, dtype=np.float64), max_depth=np.float64(MAX_DEPTH))
    print("wrote %s: %d bytes" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
