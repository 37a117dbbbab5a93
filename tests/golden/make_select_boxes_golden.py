"""Generate tests/golden/select_boxes.npz, select_boxes_label.txt and select_boxes_calib.txt.

Runs where the reference tree is mounted and scipy is installed:

    python tests/golden/make_select_boxes_golden.py <reference tree>      (or VOTENET_REFERENCE=<reference tree>)

Every expected value comes from the reference's own code, imported and called: SUNObject3d and SUNRGBD_Calibration parse
the text, project_upright_depth_to_image / project_upright_depth_to_upright_camera / compute_box_3d / extract_pc_in_box3d
(scipy Delaunay) do the geometry.  dataset.py cannot be imported (mayavi, tensorpack, cv2 at module level), so the
per-object loop of dataset.py:237-283 is restated around those calls; cv2, which sunutils imports and these functions
never use, is an empty stand-in module.  The count recorded per object is the number of frustum points inside the hull.
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

WHITELIST = ("bed", "table", "sofa", "chair", "toilet", "desk", "dresser", "night_stand", "bookshelf", "bathtub")  # dataset.py:159
N_OUT = 1280
K0 = np.array([[529.5, 0.0, 365.0], [0.0, 529.5, 265.0], [0.0, 0.0, 1.0]])


def rot(ax, t):
    c, s = np.cos(t), np.sin(t)
    m = {0: [[1, 0, 0], [0, c, -s], [0, s, c]], 1: [[c, 0, s], [0, 1, 0], [-s, 0, c]], 2: [[c, -s, 0], [s, c, 0], [0, 0, 1]]}
    return np.array(m[ax], float)


def calib_text(rtilt, k):
    """Two lines, nine numbers each, column-major (sunutils.py:59-64)."""
    return " ".join(repr(float(x)) for x in rtilt.flatten(order="F")) + "\n" + " ".join(repr(float(x)) for x in k.flatten(order="F")) + "\n"


def load_calib(text, keep=None):
    path = keep
    if path is None:
        fd, path = tempfile.mkstemp(suffix=".txt")
        os.close(fd)
    with open(path, "w") as f:
        f.write(text)
    cal = SU.SUNRGBD_Calibration(path)
    if keep is None:
        os.remove(path)
    return cal


def label_line(name, box2d, centroid, l, w, h, yaw):
    """name, 2D box (x, y, width, height), centroid, w l h, a 2x2 basis (unused), orientation: sunutils.py:10-34."""
    xmin, ymin, xmax, ymax = box2d
    c, s = np.cos(yaw), np.sin(yaw)
    vals = [xmin, ymin, xmax - xmin, ymax - ymin, centroid[0], centroid[1], centroid[2], w, l, h, c, s, -s, c, c, s]
    return name + " " + " ".join(repr(float(x)) for x in vals)


def projected_box2d(cal, centroid, l, w, h, yaw, margin=10.0):
    """The image bounds of the eight corners, widened: a 2D box that contains the whole 3D box."""
    obj = SU.SUNObject3d(label_line("bed", (0, 0, 1, 1), centroid, l, w, h, yaw))
    c2d, _ = SU.compute_box_3d(obj, cal)
    return (c2d[:, 0].min() - margin, c2d[:, 1].min() - margin, c2d[:, 0].max() + margin, c2d[:, 1].max() + margin)


def reference_scene(pc, cal, objects):
    """dataset.py:185-189,237-283 around the reference's functions.  pc: the subsampled (n, >=3) float64 rows."""
    pc_cam = np.zeros_like(pc)
    pc_cam[:, 0:3] = cal.project_upright_depth_to_upright_camera(pc[:, 0:3])
    pc_cam[:, 3:] = pc[:, 3:]
    with np.errstate(divide="ignore", invalid="ignore"):
        pc_img, _ = cal.project_upright_depth_to_image(pc)
    n, nobj = len(pc), len(objects)
    inside = np.zeros((nobj, n), bool)
    n_inside = np.zeros(nobj, np.int32)
    status = np.zeros(nobj, np.int32)
    center, size, heading, cls = [], [], [], []
    for o, obj in enumerate(objects):
        if obj.classname not in WHITELIST:
            status[o] = 1
            continue
        xmin, ymin, xmax, ymax = obj.box2d
        fov = (pc_img[:, 0] < xmax) & (pc_img[:, 0] >= xmin) & (pc_img[:, 1] < ymax) & (pc_img[:, 1] >= ymin)
        pc_fov = pc_cam[fov, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            _, c3d = SU.compute_box_3d(obj, cal)
        c3d = cal.project_upright_depth_to_upright_camera(c3d)
        if np.max(c3d[:, 1]) - np.min(c3d[:, 1]) < 1e-7:
            status[o] = 2
            continue
        _, inds = SU.extract_pc_in_box3d(pc_fov, c3d)
        inside[o, np.nonzero(fov)[0][inds]] = True
        n_inside[o] = int(inds.sum())
        if n_inside[o] < 5:
            status[o] = 3
            continue
        center.append((c3d[0, :] + c3d[6, :]) / 2)
        size.append(np.array([2 * obj.l, 2 * obj.w, 2 * obj.h]))
        heading.append(obj.heading_angle)
        cls.append(WHITELIST.index(obj.classname))
    return {"inside": inside, "n_inside": n_inside, "status": status, "center": np.array(center).reshape(-1, 3),
            "size": np.array(size).reshape(-1, 3), "heading": np.array(heading, float), "cls": np.array(cls, np.int32)}


def cloud(rng, n, cols, y_lo=0.6):
    pts = np.column_stack([rng.uniform(-3, 3, n), rng.uniform(y_lo, 6.5, n), rng.uniform(-1.5, 1.5, n)])
    extra = rng.integers(0, 256, (n, cols - 3)) / 255.0   # colour-like extra columns
    return np.column_stack([pts, extra])


def random_objects(rng, cal, count, names):
    lines = []
    for i in range(count):
        cen = np.array([rng.uniform(-2.2, 2.2), rng.uniform(2.0, 5.5), rng.uniform(-0.8, 0.8)])
        l, w, h = rng.uniform(0.25, 0.9, 3)
        yaw = rng.uniform(-np.pi, np.pi)
        lines.append(label_line(names[i % len(names)], projected_box2d(cal, cen, l, w, h, yaw), cen, l, w, h, yaw))
    return lines


def main():
    rng = np.random.default_rng(20240607)
    tilt = rot(0, 0.21) @ rot(1, -0.04) @ rot(2, 0.03)
    scenes = []  # (raw, choice, calib text, label lines)

    # ---- scene 0: the text fixtures.  Tilted camera; every reject reason; boxes holding exactly 3, 4, 5, 6 points; a 2D box
    # that cuts its 3D box
    cal_text0 = calib_text(tilt, K0)
    cal = load_calib(cal_text0, os.path.join(HERE, "select_boxes_calib.txt"))
    n_raw, cols = 1900, 6
    raw = cloud(rng, n_raw, cols)
    choice = rng.choice(n_raw, N_OUT, replace=False)
    lines = [label_line("bed", projected_box2d(cal, (-1.2, 3.0, -0.6), 1.0, 0.8, 0.5, 0.4), (-1.2, 3.0, -0.6), 1.0, 0.8, 0.5, 0.4),
             label_line("chair", projected_box2d(cal, (1.4, 2.6, -0.5), 0.45, 0.4, 0.7, -2.1), (1.4, 2.6, -0.5), 0.45, 0.4, 0.7, -2.1),
             label_line("lamp", projected_box2d(cal, (0.3, 3.2, 0.2), 0.6, 0.6, 0.8, 0.0), (0.3, 3.2, 0.2), 0.6, 0.6, 0.8, 0.0),
             label_line("table", projected_box2d(cal, (0.2, 4.0, -0.4), 0.9, 0.7, 0.0, 1.0), (0.2, 4.0, -0.4), 0.9, 0.7, 0.0, 1.0),
             label_line("desk", projected_box2d(cal, (0.2, 4.0, -0.4), 0.9, 0.7, 4e-8, 1.0), (0.2, 4.0, -0.4), 0.9, 0.7, 4e-8, 1.0),
             label_line("sofa", projected_box2d(cal, (0.2, 4.0, -0.4), 0.9, 0.7, 6e-8, 1.0), (0.2, 4.0, -0.4), 0.9, 0.7, 6e-8, 1.0)]
    # count boxes in a strip cleared of cloud points (y in [5.0, 6.5], z in [0.6, 1.5]); their points are placed, and sit on
    # rows the subsample takes
    strip = (raw[:, 1] > 5.0) & (raw[:, 2] > 0.6)
    raw[strip, 2] -= 1.2
    row = 0
    for i, (name, k) in enumerate((("toilet", 3), ("dresser", 4), ("night_stand", 5), ("bookshelf", 6))):
        cen = np.array([-2.1 + 1.4 * i, 5.8, 1.1])
        l, w, h, yaw = 0.3, 0.25, 0.2, 0.5 * i - 0.6
        lines.append(label_line(name, projected_box2d(cal, cen, l, w, h, yaw), cen, l, w, h, yaw))
        R = rot(2, yaw)
        for _ in range(k):
            raw[choice[row], :3] = cen + R @ (rng.uniform(-0.6, 0.6, 3) * np.array([l, w, h]))
            row += 1
    # the cut: a 2D box that covers the left half of the projected 3D box only
    cen, (l, w, h, yaw) = np.array([2.0, 4.2, 0.0]), (0.8, 0.8, 0.9, 0.2)
    x0, y0, x1, y1 = projected_box2d(cal, cen, l, w, h, yaw)
    lines.append(label_line("bathtub", (x0, y0, (x0 + x1) / 2, y1), cen, l, w, h, yaw))
    with open(os.path.join(HERE, "select_boxes_label.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    scenes.append((raw, choice, cal_text0, lines))

    # ---- scene 1: identity Rtilt, points behind the camera (uv2 < 0), a box that straddles the camera plane under an
    # image-sized 2D box, a few ordinary boxes
    text = calib_text(np.eye(3), K0)
    cal = load_calib(text)
    raw = cloud(rng, 1700, 4, y_lo=-2.0)
    lines = [label_line("sofa", (-1e5, -1e5, 1e5, 1e5), (0.1, 0.2, 0.0), 1.0, 1.1, 1.0, 0.3)]
    lines += random_objects(rng, cal, 5, ("bed", "desk", "monitor", "chair"))
    scenes.append((raw, rng.choice(len(raw), N_OUT, replace=False), text, lines))

    # ---- scene 2: more objects than one pass of the kernel holds in LDS
    text = calib_text(rot(0, -0.15) @ rot(2, 0.05), K0 * np.array([[1.1], [0.9], [1.0]]))
    cal = load_calib(text)
    raw = cloud(rng, 1600, 5)
    lines = random_objects(rng, cal, 70, WHITELIST + ("picture", "box"))
    scenes.append((raw, rng.choice(len(raw), N_OUT, replace=False), text, lines))

    # ---- scene 3: keeps nothing (one name outside the whitelist, one box above the cloud)
    raw = cloud(rng, 1500, 3)
    lines = [label_line("whiteboard", projected_box2d(cal, (0, 3, 0), 0.5, 0.5, 0.5, 0), (0, 3, 0), 0.5, 0.5, 0.5, 0),
             label_line("table", projected_box2d(cal, (0, 3, 2.6), 0.5, 0.5, 0.5, 0), (0, 3, 2.6), 0.5, 0.5, 0.5, 0)]
    scenes.append((raw, rng.choice(len(raw), N_OUT, replace=False), text, lines))

    # ---- scene 4: nothing labelled
    scenes.append((cloud(rng, 1400, 3), rng.choice(1400, N_OUT, replace=False), cal_text0, []))

    # ---- scene 5: a generic tilted scene
    text = calib_text(rot(1, 0.07) @ rot(0, 0.3), K0)
    cal = load_calib(text)
    raw = cloud(rng, 2000, 6)
    lines = random_objects(rng, cal, 8, WHITELIST)
    scenes.append((raw, rng.choice(len(raw), N_OUT, replace=False), text, lines))

    out = {"n_out": np.int64(N_OUT), "b": np.int64(len(scenes))}
    obj_arrays = {k: [] for k in ("cls", "box2d", "centroid", "half_extent", "heading")}
    obj_off, rt, km = [0], [], []
    for s, (raw, choice, text, lines) in enumerate(scenes):
        cal = load_calib(text)
        objects = [SU.SUNObject3d(line) for line in lines]
        rt.append(cal.Rtilt), km.append(cal.K)
        for o in objects:
            obj_arrays["cls"].append(WHITELIST.index(o.classname) if o.classname in WHITELIST else -1)
            obj_arrays["box2d"].append(o.box2d), obj_arrays["centroid"].append(o.centroid)
            obj_arrays["half_extent"].append([o.l, o.w, o.h]), obj_arrays["heading"].append(o.heading_angle)
        obj_off.append(obj_off[-1] + len(objects))
        raw32 = raw.astype(np.float32)
        out["raw64_%d" % s], out["raw32_%d" % s], out["choice_%d" % s] = raw, raw32, choice.astype(np.int32)
        for tag, cloud_ in (("f64", raw), ("f32", raw32.astype(np.float64))):
            r = reference_scene(np.ascontiguousarray(cloud_[choice]), cal, objects)
            out["inside_%s_%d" % (tag, s)] = np.packbits(r["inside"], axis=1)
            for k in ("n_inside", "status", "center", "size", "heading", "cls"):
                out["%s_%s_%d" % (k, tag, s)] = r[k]
            print("scene %d %s: %d objects, status %s, n_inside %s" % (s, tag, len(objects), np.bincount(r["status"], minlength=4),
                                                                      r["n_inside"][:12]))
    out["Rtilt"], out["K"], out["obj_offset"] = np.array(rt), np.array(km), np.array(obj_off, np.int64)
    out["obj_cls"] = np.array(obj_arrays["cls"], np.int32)
    out["obj_box2d"] = np.array(obj_arrays["box2d"], float).reshape(-1, 4)
    out["obj_centroid"] = np.array(obj_arrays["centroid"], float).reshape(-1, 3)
    out["obj_half_extent"] = np.array(obj_arrays["half_extent"], float).reshape(-1, 3)
    out["obj_heading"] = np.array(obj_arrays["heading"], float)
    path = os.path.join(HERE, "select_boxes.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
