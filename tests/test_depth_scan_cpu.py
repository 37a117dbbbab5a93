"""CPU: the rule of include/votenet_depth_scan.h as tests/depth_scan_ref.py restates it, against the reference's own geometry
(tests/golden/depth_scan.npz, made by tests/golden/make_depth_scan_golden.py from sunutils.SUNRGBD_Calibration), and the argument
checks of libvotenet_depth.so, which launch nothing.  The device's bytes are compared with the restatement in
tests/test_gpu_depth_scan.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_scan_ref as R  # noqa: E402


def half_ulp32(v):
    """Half the spacing of float32 in the binade of |v| (float64): the most that one rounding to nearest moves v."""
    _, e = np.frexp(np.abs(np.asarray(v, np.float64)))  # |v| = m 2^e, 0.5 <= m < 1
    return np.ldexp(0.5, e - 24)


# ------------------------------------------------------------------ the restatement against the reference
def test_restatement_matches_the_reference_geometry_to_one_rounding(golden):
    """Each coordinate within half a float32 ulp of the reference's float64 value plus 1e-12: the restatement's fixed summation order
    and BLAS's differ at the double level only."""
    g = golden("depth_scan")
    image, rtilt, k, exp = g["image"], g["rtilt"], g["k"], g["points"]
    assert image.shape == (53, 61) and image.dtype == np.uint16 and exp.dtype == np.float64
    zeros = float((image == 0).mean())
    assert 0.2 < zeros < 0.4 and abs(np.linalg.det(rtilt) - 1) < 1e-12 and abs(rtilt[1, 2]) > 0.1 and abs(rtilt[0, 1]) > 0.05  # tilted
    from votenet_amd import sunrgbd
    rt2, k2 = sunrgbd.parse_calib(str(g["calib_text"]))  # the calibration as this project parses the reference's file
    assert np.array_equal(rt2, rtilt) and np.array_equal(k2, k)
    got = R.scan_one(image, rtilt, k, encoding="sunrgbd", pixel_origin=1.0, max_depth=float(g["max_depth"]))
    assert got.dtype == np.float32 and got.shape == exp.shape == (int((image != 0).sum()), 3)
    diff = np.abs(got.astype(np.float64) - exp)
    bound = half_ulp32(exp) + 1e-12
    worst = int(np.argmax(diff / bound))
    print("max difference %.3g at |v| <= %.3f; closest to its bound: %.3g of %.3g; %d of %d equal after rounding"
          % (diff.max(), np.abs(exp).max(), diff.flat[worst], bound.flat[worst], int((got == exp.astype(np.float32)).sum()), got.size))
    assert (diff <= bound).all()
    assert (R.metres(R.decode(image[image != 0], 0), 8.0) == 8.0).sum() > 50  # the clamp took part


def test_round_trip_through_the_reference_projection():
    """project_upright_depth_to_image (restated) of the scan returns the 1-based pixel within 1e-3 px and z within 1e-6."""
    rng = np.random.default_rng(5)
    h, w = 48, 64
    rtilt, k = R.tilted_calib(rng, h, w)
    image = R.random_depth(rng, h, w, "sunrgbd")
    for origin in (1.0, 0.0):
        pts = R.scan_one(image, rtilt, k, pixel_origin=origin)
        uv, z = R.project_upright_depth_to_image(pts, rtilt, k)
        row, col = np.nonzero(image != 0)
        zz = R.metres(R.decode(image[row, col], 0))
        du, dv, dz = np.abs(uv[:, 0] - (col + origin)).max(), np.abs(uv[:, 1] - (row + origin)).max(), np.abs(z - zz).max()
        print("pixel_origin %g: |du| %.3g, |dv| %.3g px, |dz| %.3g" % (origin, du, dv, dz))
        assert du < 1e-3 and dv < 1e-3 and dz < 1e-6


def test_decode_table_for_every_pixel_value():
    p = np.arange(65536, dtype=np.uint32)
    d0, d1 = R.decode(p.astype(np.uint16), 0), R.decode(p.astype(np.uint16), 1)
    assert d0.dtype == d1.dtype == np.uint16
    assert np.array_equal(d0, ((p >> 3) | ((p & 7) << 13)).astype(np.uint16))  # the rotation, written the other way
    assert np.array_equal(d1, p.astype(np.uint16))
    assert np.array_equal(d0 != 0, p != 0) and np.array_equal(d1 != 0, p != 0)
    assert np.array_equal(R.decode(R.encode(p.astype(np.uint16), 0), 0), p.astype(np.uint16))
    for d in (d0, d1):
        for max_depth in (8.0, 3.3335):
            z = R.metres(d, max_depth)
            exact = d.astype(np.float64) / 1000.0
            assert z.max() == max_depth and np.array_equal(z, np.minimum(exact, max_depth)) and (z[exact <= max_depth] == exact[exact <= max_depth]).all()
    # a one-row image of all 65 536 values: the valid pixels are all but value 0, in order, at their depths
    img = p.astype(np.uint16).reshape(1, -1)
    pts = R.scan_one(img, np.eye(3), np.array([[500.0, 0, 0], [0, 500.0, 0], [0, 0, 1.0]]), encoding=1)
    assert pts.shape == (65535, 3) and np.array_equal(pts[:, 1], np.minimum(np.arange(1, 65536) / 1000.0, 8.0).astype(np.float32))


def test_load_depth_png_round_trip(tmp_path):
    from PIL import Image
    from votenet_amd import InvalidArgumentError, depth_scan
    d = R.random_depth(np.random.default_rng(1), 48, 64, "sunrgbd")
    Image.fromarray(d).save(str(tmp_path / "d.png"))
    back = depth_scan.load_depth_png(str(tmp_path / "d.png"))
    assert back.dtype == np.uint16 and back.flags.c_contiguous and np.array_equal(back, d) and d.max() > 40000
    Image.fromarray(np.zeros((4, 4, 3), np.uint8)).save(str(tmp_path / "c.png"))
    with pytest.raises(InvalidArgumentError, match="not a single-channel 16-bit image"):
        depth_scan.load_depth_png(str(tmp_path / "c.png"))


# ------------------------------------------------------------------ the library's argument checks
def _args(b=2, h=(4, 5), w=(6, 3), rgb=False):
    hw = np.ascontiguousarray(np.stack([h[:b], w[:b]], 1), dtype=np.int32)
    off = np.zeros(b + 1, np.int64)
    off[1:] = np.cumsum(hw[:, 0].astype(np.int64) * hw[:, 1])
    total = int(off[-1])
    a = dict(b=b, depth=np.ones(total + 8, np.uint16), rgb=np.ones(3 * total + 8, np.uint8) if rgb else None, off=off, hw=hw,
             rtilt=np.ascontiguousarray(np.tile(np.eye(3).reshape(1, 9), (b, 1))),
             k=np.ascontiguousarray(np.tile(np.array([[500.0, 0, 3, 0, 500.0, 2, 0, 0, 1]]), (b, 1))), encoding=0, origin=1.0, max_depth=8.0,
             raw=np.zeros((total, 6), np.float32), stride=6 if rgb else 3, cap=total, off_dev=np.zeros(b + 1, np.int64),
             ws=np.zeros(4096, np.int32))
    a["ws_bytes"] = a["ws"].nbytes
    return a


def _call(lib, a):
    hp = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)
    return lib.votenet_depth_scan(a["b"], hp(a["depth"]), hp(a["rgb"]), hp(a["off"]), hp(a["hw"]), hp(a["rtilt"]), hp(a["k"]), a["encoding"],
                                  a["origin"], a["max_depth"], hp(a["raw"]), a["stride"], a["cap"], hp(a["off_dev"]), hp(a["ws"]),
                                  a["ws_bytes"], None)


def test_invalid_arguments_return_status_1_and_launch_nothing(hiplib):
    """Host pointers throughout: a launch would fault, a status 1 before any launch does not.  Every buffer is as it was afterwards."""
    from votenet_amd import _lib as L
    lib = L.side_lib("depth")
    need = lib.votenet_depth_scan_workspace_bytes(2, 4 * 6 + 5 * 3)

    def bad(expect, **change):
        a = _args(rgb=change.pop("rgb", False))
        for key, val in change.items():
            if callable(val):
                val(a)
            else:
                a[key] = val
        assert _call(lib, a) == 1, expect
        text = lib.votenet_depth_scan_last_error().decode()
        assert expect in text, (expect, text)
        assert (a["raw"] is None or not a["raw"].any()) and (a["off_dev"] is None or not a["off_dev"].any()) and not a["ws"].any()
        with pytest.raises(L.InvalidArgumentError, match="depth_scan"):
            L.check(1, side="depth")

    bad("scenes per call, got b = 0", b=0)
    bad("scenes per call, got b = -1", b=-1)
    bad("scenes per call, got b = 33", b=33)
    bad("scene 1 is 0 x 3 pixels", edit=lambda a: a["hw"].__setitem__((1, 0), 0))
    bad("scene 0 is 4 x -6 pixels", edit=lambda a: a["hw"].__setitem__((0, 1), -6))
    bad("pix_offset gives it 25", edit=lambda a: a["off"].__setitem__(1, 25))
    bad("pix_offset must start at 0", edit=lambda a: a["off"].__iadd__(1))
    bad("raw_stride must be 3 without colour, got 6", stride=6)
    bad("raw_stride must be 3 without colour, got 4", stride=4)
    bad("raw_stride must be 6 with colour, got 3", rgb=True, stride=3)
    bad("workspace of %d bytes, need %d" % (need - 1, need), ws_bytes=need - 1)
    bad("workspace of 0 bytes", ws_bytes=0)
    bad("scene 1 has K[0,0] = 0", edit=lambda a: a["k"].__setitem__((1, 0), 0.0))
    bad("scene 0 has K[0,0] = 500, K[1,1] = 0", edit=lambda a: a["k"].__setitem__((0, 4), 0.0))
    bad("encoding must be 0", encoding=2)
    bad("encoding must be 0", encoding=-1)
    bad("raw_capacity_rows must be >= 0", cap=-1)
    bad("null raw with room for 39 rows", raw=None)
    bad("null pointer", off_dev=None)


def test_workspace_bytes_is_monotone_and_covers_every_split(hiplib):
    from votenet_amd import _lib as L
    from votenet_amd import depth_scan
    lib = L.side_lib("depth")
    wb = lib.votenet_depth_scan_workspace_bytes
    pixels = [0, 1, 2047, 2048, 2049, 386900, 8 * 386900, 2 ** 31 - 1]
    for b in (1, 2, 17, 32):
        vals = [wb(b, n) for n in pixels]
        assert vals == sorted(vals) and vals[0] > 0
        assert all(wb(b, n) <= wb(b + 1, n) for n in pixels)
    # one int per tile of every scene, whatever the split of the pixels and wherever a scene starts in its 16-byte group
    T = depth_scan.TILE_PIXELS
    for n in (1, T - 1, T, T + 1, 3 * T + 5):
        most = max((head + n + T - 1) // T for head in range(8))
        assert wb(3, n) >= 3 * most * 4
