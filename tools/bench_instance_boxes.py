#!/usr/bin/env python3
"""Time the ground-truth boxes from instance-labelled points (libvotenet_instbox.so) on the GPU: 8 scenes of 40 000 points, k = 256.

    python tools/bench_instance_boxes.py [--iters 2000] [--warmup 50] [--out profiles/instance_boxes_bench.txt]

Prints, and appends to --out when given:
  * votenet_instance_boxes (memset, tile pass, finish): microseconds per batch by device events around `iters` calls on buffers
    allocated before, after a warm-up, and the bytes the algorithm needs -- 12 B of coordinates and 4 B of instance id read per point --
    over that time, as a fraction of the chip's 8 TB/s; votenet_instance_point_box likewise;
  * the same extents and counts as plain torch ops on the device (scatter_reduce_ amin / amax and bincount over scene * k + id),
    checked equal to the library's before they are timed, timed the same way;
  * boxes_from_labels, the whole Python entry with its allocations and its one read-back, by the host clock.
Needs a GPU: there is no CPU path to time."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import instance_boxes_ref as R  # noqa: E402

from votenet_amd import _lib as L  # noqa: E402
from votenet_amd import instance_boxes as IB  # noqa: E402

B, N, K = 8, 40000, 256
PEAK = 8.0e12  # bytes/s


def scenes(rng):
    """60 to 120 instances per scene of very different sizes, a third of the points unlabelled, in random order (a subsample's): every
    tile meets every instance.  A few holes."""
    pts = (rng.normal(size=(B, N, 3)) * [3.0, 1.0, 3.0]).astype(np.float32)
    inst = np.empty((B, N), np.int32)
    for s in range(B):
        n_inst = int(rng.integers(60, 121))
        w = rng.random(n_inst) ** 3 + 0.01
        inst[s] = rng.choice(n_inst, N, p=w / w.sum())
        pts[s] += (rng.random((n_inst, 3)) * 8)[inst[s]].astype(np.float32)
    inst[rng.random((B, N)) < 0.33] = -1
    pts[rng.random((B, N)) < 0.001] = np.nan
    sem = (np.abs(inst) % 18).astype(np.int32)
    class_map = (np.arange(18) % 11 - 1).astype(np.int32)  # -1 .. 9
    return pts, inst, sem, class_map


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
    assert torch.cuda.is_available(), "bench_instance_boxes needs a GPU"
    dev = torch.device("cuda:0")
    pts_h, inst_h, sem_h, cm_h = scenes(np.random.default_rng(0))
    pts, inst, sem, cm = (torch.from_numpy(x).to(dev) for x in (pts_h, inst_h, sem_h, cm_h))
    # the launchers on buffers allocated once
    lib = L.side_lib("instbox")
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    rows = [f64(B * K, 3), f64(B * K, 3), f64(B * K), i32(B * K), i32(B * K), i32(B * K)]
    kept, slot, status, count, ignored, point_box = i32(B), i32(B, K), i32(B, K), i32(B, K), i32(B, 3), i32(B, N)
    need = lib.votenet_instance_boxes_workspace_bytes(B, K)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    st = L.stream_ptr()

    def ours():
        L.check(lib.votenet_instance_boxes(B, N, K, len(cm_h), 10, 5, pts.data_ptr(), inst.data_ptr(), sem.data_ptr(), cm.data_ptr(),
                                           *[t.data_ptr() for t in rows], kept.data_ptr(), slot.data_ptr(), status.data_ptr(),
                                           count.data_ptr(), ignored.data_ptr(), ws.data_ptr(), need, st), side="instbox")

    def ours_point_box():
        L.check(lib.votenet_instance_point_box(B, N, K, pts.data_ptr(), inst.data_ptr(), slot.data_ptr(), point_box.data_ptr(), st),
                side="instbox")
    us = timed(ours, a.iters, a.warmup)
    us_pb = timed(ours_point_box, a.iters, a.warmup)
    exp = R.boxes_from_labels(pts_h, inst_h, sem_h, cm_h, k=K, n_class=10, min_points=5)
    nk = int(exp["box_offset"][-1])
    got = {"center": rows[0][:nk], "size": rows[1][:nk], "cls": rows[3][:nk], "n_points": rows[5][:nk], "status": status, "inst_count": count,
           "ignored": ignored, "point_box": point_box}
    bad = R.same_bytes({key: v.cpu().numpy() for key, v in got.items()}, exp, tuple(got))
    assert not bad and int(kept.sum()) == nk, "the library differs from the restatement in %s" % bad
    # the same extents and counts in torch ops: one table of B * K entries and a slot for the points that do not take part
    scene = torch.arange(B, device=dev)[:, None] * K

    def plain():
        part = (inst >= 0) & (inst < K) & torch.isfinite(pts).all(-1)
        idx = torch.where(part, scene + inst, B * K).reshape(-1)
        idx3 = idx[:, None].expand(-1, 3)
        flat = pts.reshape(-1, 3)
        lo = torch.full((B * K + 1, 3), float("inf"), device=dev).scatter_reduce_(0, idx3, flat, "amin")
        hi = torch.full((B * K + 1, 3), float("-inf"), device=dev).scatter_reduce_(0, idx3, flat, "amax")
        return lo, hi, torch.bincount(idx, minlength=B * K + 1)
    lo, hi, cnt = plain()
    same = bool(torch.equal(cnt[:-1].reshape(B, K).to(torch.int32), count))
    keep = torch.from_numpy((exp["slot"] >= 0).reshape(-1)).to(dev)
    lo64, hi64 = lo[:-1][keep].double(), hi[:-1][keep].double()
    same = same and bool(torch.equal((lo64 + hi64) * 0.5, rows[0][:nk])) and bool(torch.equal(hi64 - lo64, rows[1][:nk]))
    us_torch = timed(plain, max(a.iters // 10, 5), max(a.warmup // 10, 2))
    # the whole Python entry, allocations and read-back included
    IB.boxes_from_labels(pts, inst, sem, cm, k=K, min_points=5)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        IB.boxes_from_labels(pts, inst, sem, cm, k=K, min_points=5)
    torch.cuda.synchronize()
    us_entry = (time.perf_counter() - t0) / 20 * 1e6
    model = B * N * 16
    lines = [
        "instance_boxes bench: %d scenes of %d points, k = %d, %d boxes kept of %d instances present, %s, %d iterations after %d"
        % (B, N, K, nk, int((exp["inst_count"] > 0).sum()), torch.cuda.get_device_name(0), a.iters, a.warmup),
        "votenet_instance_boxes (memset, tile pass, finish): %.1f us per batch; %.1f MB by the model (16 B / point) = %.2f TB/s = %.1f %% of 8 TB/s"
        % (us, model / 1e6, model / us / 1e6, 100.0 * model / (us * 1e-6) / PEAK),
        "votenet_instance_point_box (one launch): %.1f us per batch" % us_pb,
        "the same extents and counts as torch ops on the device (scatter_reduce_ amin / amax, bincount): %.1f us per batch, %.1f x; equal to the library's: %s"
        % (us_torch, us_torch / us, same),
        "boxes_from_labels (allocations, three launches, the read-back of kept): %.0f us per batch by the host clock" % us_entry,
    ]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
