"""Host text parsers for SUN RGB-D scenes as the reference reads them (sunutils.py:10-34 label lines, :59-68 calibration).

Text in, arrays out: no file-system walking, no image or .mat reading.  What the arrays feed is
input_pipeline.select_boxes / build_batch, which do the per-point work of dataset.py:237-283 on the device.
"""
import numpy as np

# dataset.py:31-32 type2class, which is also the whitelist of dataset.py:159-160 and the row order of synth.MEAN_SIZES
CLASS_NAMES = ("bed", "table", "sofa", "chair", "toilet", "desk", "dresser", "night_stand", "bookshelf", "bathtub")
_CLASS_ID = {n: i for i, n in enumerate(CLASS_NAMES)}

OBJECT_FIELDS = (("cls", 0, np.int32), ("box2d", 4, np.float64), ("centroid", 3, np.float64), ("half_extent", 3, np.float64),
                 ("heading", 0, np.float64))


def _empty():
    return {k: np.zeros((0, w) if w else (0,), dt) for k, w, dt in OBJECT_FIELDS}


def parse_label(text):
    """One scene's label file (one object per line: name, 2D box x y w h, centroid, w l h, basis, orientation) -> dict of
    per-object arrays: cls (int32; -1 for a name outside CLASS_NAMES), box2d (xmin, ymin, xmax, ymax), centroid,
    half_extent (l, w, h) and heading, float64, plus `names`."""
    out = {k: [] for k, _, _ in OBJECT_FIELDS}
    names = []
    for line in text.splitlines():
        line = line.rstrip()
        if not line:
            continue
        data = line.split(" ")
        d = [float(x) for x in data[1:]]                      # d[i] is the reference's data[i + 1]
        names.append(data[0])
        out["cls"].append(_CLASS_ID.get(data[0], -1))
        out["box2d"].append([d[0], d[1], d[0] + d[2], d[1] + d[3]])          # sunutils.py:15-19
        out["centroid"].append([d[4], d[5], d[6]])                           # :20
        out["half_extent"].append([d[8], d[7], d[9]])                        # :22-24: l = data[9], w = data[8], h = data[10]
        out["heading"].append(-1 * np.arctan2(d[15], d[14]))                 # :31-34
    res = _empty()
    if names:
        res = {k: np.asarray(out[k], dt).reshape((-1, w) if w else (-1,)) for k, w, dt in OBJECT_FIELDS}
    res["names"] = names
    return res


def parse_calib(text):
    """Calibration file: line 0 Rtilt, line 1 K, nine numbers each in column-major order (sunutils.py:59-64).
    -> (Rtilt, K), (3, 3) float64, C-contiguous."""
    lines = [line.rstrip() for line in text.splitlines()]
    rtilt = np.array([float(x) for x in lines[0].split(" ")])
    k = np.array([float(x) for x in lines[1].split(" ")])
    return (np.ascontiguousarray(np.reshape(rtilt, (3, 3), order="F")), np.ascontiguousarray(np.reshape(k, (3, 3), order="F")))


def pack_objects(scenes):
    """list of parse_label results (one per scene, possibly without objects) -> dict of the concatenated arrays plus
    obj_offset, host int64 (b + 1): the `objects` argument of input_pipeline.select_boxes."""
    off = np.zeros(len(scenes) + 1, np.int64)
    off[1:] = np.cumsum([len(s["cls"]) for s in scenes])
    res = {k: np.ascontiguousarray(np.concatenate([np.asarray(s[k], dt).reshape((-1, w) if w else (-1,)) for s in scenes] or
                                                  [_empty()[k]], 0)) for k, w, dt in OBJECT_FIELDS}
    res["obj_offset"] = off
    return res
