#!/usr/bin/env python3
"""Time the raw scan from the depth image (libvotenet_depth.so) on the GPU: 8 scenes of 530 x 730 pixels with colour.

    python tools/bench_depth_scan.py [--iters 2000] [--warmup 50] [--out profiles/depth_scan_bench.txt]

Prints, and appends to --out when given:
  * votenet_depth_scan: microseconds per batch (device events around `iters` calls on buffers allocated before, after a warm-up), and
    the bytes the algorithm needs -- 2 B read per pixel in each of the two passes, 24 B written per valid pixel; the colour bytes read,
    3 B per pixel, are reported beside it -- over that time, as a fraction of the chip's 8 TB/s;
  * the same job as plain torch ops on the device (decode, mask, nonzero, float64 arithmetic, one rounding), timed the same way;
  * np.loadtxt of ONE scene's scan as text (the reference's input, sunutils.py:178-180), host seconds.
Needs a GPU: there is no CPU path to time."""
import argparse
import ctypes
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import depth_scan_ref as R  # noqa: E402

from votenet_amd import _lib as L  # noqa: E402
from votenet_amd import depth_scan  # noqa: E402
from votenet_amd import input_pipeline as IP  # noqa: E402

B, H, W = 8, 530, 730
PEAK = 8.0e12  # bytes/s


def torch_scan(d, c, rt, km, h, w, origin=1.0, max_depth=8.0):
    """One scene with torch ops: d (h*w) int32 pixel values, c (h*w, 3) uint8 on the device -> (n, 6) float32."""
    d16 = ((d >> 3) | (d << 13)) & 0xffff
    idx = torch.nonzero(d16).reshape(-1)
    z = torch.clamp(d16[idx].to(torch.float64) / 1000.0, max=max_depth)
    u = (idx % w).to(torch.float64) + origin
    v = (idx // w).to(torch.float64) + origin
    x = ((u - km[0, 2]) * z) / km[0, 0]
    y = ((v - km[1, 2]) * z) / km[1, 1]
    p = (x, z, -y)
    cols = [((rt[i, 0] * p[0] + rt[i, 1] * p[1]) + rt[i, 2] * p[2]).to(torch.float32) for i in range(3)]
    rgb = (c[idx].to(torch.float64) / 255.0).to(torch.float32)
    return torch.cat([torch.stack(cols, 1), rgb], 1)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters  # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_depth_scan needs a GPU"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    depth = [R.random_depth(rng, H, W, "sunrgbd", zeros=0.15) for _ in range(B)]
    rgb = [rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(B)]
    calib = [R.tilted_calib(rng, H, W) for _ in range(B)]
    # the launcher on buffers allocated once
    lib = L.side_lib("depth")
    d = torch.from_numpy(np.concatenate([x.reshape(-1) for x in depth]).view(np.int16)).to(dev)
    c = torch.from_numpy(np.concatenate([x.reshape(-1) for x in rgb])).to(dev)
    hw = np.ascontiguousarray([[H, W]] * B, dtype=np.int32)
    off = np.arange(B + 1, dtype=np.int64) * (H * W)
    rt, km = IP._calib_arrays(calib, B, "bench")
    total = int(off[-1])
    raw = torch.empty((total, 6), dtype=torch.float32, device=dev)
    off_dev = torch.empty((B + 1,), dtype=torch.int64, device=dev)
    need = lib.votenet_depth_scan_workspace_bytes(B, total)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    st = L.stream_ptr()
    hp = lambda x: x.ctypes.data_as(ctypes.c_void_p)

    def ours():
        L.check(lib.votenet_depth_scan(B, d.data_ptr(), c.data_ptr(), hp(off), hp(hw), hp(rt), hp(km), 0, 1.0, 8.0, raw.data_ptr(), 6, total,
                                       off_dev.data_ptr(), ws.data_ptr(), need, st), side="depth")
    us = timed(ours, a.iters, a.warmup)
    valid = int(off_dev.cpu()[-1])
    exp, eoff = R.scan(depth[:1], calib[:1], rgb[:1])
    assert np.array_equal(raw[:len(exp)].cpu().numpy().view(np.uint32), exp.view(np.uint32)), "scene 0 differs from the restatement"
    model = 2 * 2 * total + 24 * valid
    with_colour = model + 3 * total
    # the same job in torch ops
    di = [torch.from_numpy(x.reshape(-1).astype(np.int32)).to(dev) for x in depth]
    ci = [torch.from_numpy(x.reshape(-1, 3)).to(dev) for x in rgb]
    rtd = [torch.from_numpy(x[0]).to(dev) for x in calib]
    kmd = [torch.from_numpy(x[1]).to(dev) for x in calib]

    def plain():
        return torch.cat([torch_scan(di[s], ci[s], rtd[s], kmd[s], H, W) for s in range(B)])
    same = np.array_equal(plain()[:len(exp)].cpu().numpy().view(np.uint32), exp.view(np.uint32))
    us_torch = timed(plain, max(a.iters // 10, 5), max(a.warmup // 10, 2))
    # the whole Python entry, upload and read-back included
    t0 = time.perf_counter()
    for _ in range(5):
        depth_scan.scan_from_depth(depth, calib, rgb)
    torch.cuda.synchronize()
    us_entry = (time.perf_counter() - t0) / 5 * 1e6
    # the reference's input: one scene's scan as text
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "000001.txt")
        np.savetxt(path, exp, fmt="%.6f")
        size = os.path.getsize(path)
        t0 = time.perf_counter()
        back = np.loadtxt(path)
        s_text = time.perf_counter() - t0
    assert back.shape == exp.shape
    lines = [
        "depth_scan bench: %d scenes of %d x %d with colour, %d of %d pixels valid, %s, %d iterations after %d"
        % (B, H, W, valid, total, torch.cuda.get_device_name(0), a.iters, a.warmup),
        "votenet_depth_scan (three launches): %.1f us per batch; %.1f MB by the model (4 B / pixel + 24 B / valid pixel) = %.2f TB/s = %.1f %% of 8 TB/s"
        % (us, model / 1e6, model / us / 1e6, 100.0 * model / (us * 1e-6) / PEAK),
        "  with the colour bytes read (3 B / pixel): %.1f MB = %.2f TB/s = %.1f %% of 8 TB/s"
        % (with_colour / 1e6, with_colour / us / 1e6, 100.0 * with_colour / (us * 1e-6) / PEAK),
        "the same job as torch ops on the device (decode, mask, nonzero, float64 arithmetic): %.1f us per batch, %.1f x; bit-equal on scene 0: %s"
        % (us_torch, us_torch / us, same),
        "scan_from_depth from host arrays (upload, three launches, the read-back): %.0f us per batch" % us_entry,
        "np.loadtxt of ONE scene's text (%d lines, %.1f MB): %.2f s on the host" % (len(exp), size / 1e6, s_text),
    ]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
