"""Generate tests/golden/box_points.npz.

Runs where the reference tree is mounted and scipy is installed:

    python tests/golden/make_box_points_golden.py <reference tree>      (or VOTENET_REFERENCE=<reference tree>)

The expected membership comes from the reference's own code, imported and called as make_select_boxes_golden.py does:
sunutils.extract_pc_in_box3d (in_hull: scipy Delaunay of the eight corners, find_simplex >= 0; sunutils.py:199-209).  cv2, which
sunutils imports and this function never uses, is an empty stand-in module.  The boxes are in the decoded corner layout
(model.py:107-111; evaluator.box_corners), float32, at random centres, sizes in 0.2 .. 1.7 and headings; every box gets 2 048 points
of its own drawn over the room, a quarter of them near the box so that enough fall inside; the coordinates are multiples of 2^-11 (the file stays small).  Only data is written: the boxes, the
points and the reference's mask (bit-packed).
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ["VOTENET_REFERENCE"]
sys.modules.setdefault("cv2", types.ModuleType("cv2"))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import sunutils as SU  # noqa: E402

from votenet_amd.evaluator import box_corners  # noqa: E402  (get_3d_box's corner order, in numpy)

NBOX, NPTS = 40, 2048
ROOM = np.array([5.0, 2.5, 5.0])


def main():
    rng = np.random.default_rng(20241018)
    center = rng.random((NBOX, 3)) * ROOM
    size = rng.uniform(0.2, 1.7, (NBOX, 3))
    heading = rng.uniform(0, 2 * np.pi, NBOX)
    boxes = box_corners(center, size, heading)  # float32
    points = (rng.random((NBOX, NPTS, 3)) * ROOM).astype(np.float32)
    near = NPTS // 4  # ... of which a quarter within the box's own neighbourhood (1.5 x its half diagonal)
    reach = 0.75 * np.linalg.norm(size, axis=1)
    points[:, :near] = (center[:, None, :] + rng.uniform(-1, 1, (NBOX, near, 3)) * reach[:, None, None]).astype(np.float32)
    points = (np.round(points * 2048.0) / 2048.0).astype(np.float32)  # a 0.5 mm grid, exact in float32: the file compresses to half
    mask = np.zeros((NBOX, NPTS), bool)
    for i in range(NBOX):
        _, inds = SU.extract_pc_in_box3d(points[i].astype(np.float64), boxes[i].astype(np.float64))
        mask[i] = inds
    print("%d boxes x %d points: %d inside (%.2f %%)" % (NBOX, NPTS, int(mask.sum()), 100.0 * mask.mean()))
    path = os.path.join(HERE, "box_points.npz")
    np.savez_compressed(path, boxes=boxes, points=points, inside=np.packbits(mask, axis=1), npts=np.int64(NPTS))
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
