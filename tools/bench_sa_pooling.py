"""Times the pooling kernels of csrc/pool_modes.hip alone with device events (needs a GPU):
    votenet_bn_relu_pool   (the pooled forward: BN + ReLU + mean / weighted sum / max / [mean | max] over each group)
    votenet_sa_pool_grad   (the pool's backward: the gradient reaching the last activation, written rows x c)
and, for comparison, votenet_bn_relu_max (thread per (group, channel quad)) on the same z.
Shapes: (a) B*npoint = 8*256 groups, k = 16, c = 128; (b) group_all, B = 8 groups, k = 20 480, c = 256.
Achieved bandwidth = the bytes the kernel must move (z read once / da written once, plus the small per-group operands) over the
measured time, and its fraction of 8 TB/s HBM.  Kernel times without launch gaps: run under `rocprofv3 --kernel-trace --stats`.

    python tools/bench_sa_pooling.py [--iters 200] [--json out.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from votenet_amd import mlp as M  # noqa: E402

HBM = 8.0e12
SHAPES = {"a_groups2048_k16_c128": (8 * 256, 16, 128), "b_group_all_8_k20480_c256": (8, 20480, 256)}


def timed(fn, iters):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sa_pooling needs a GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    res = []
    for name, (groups, k, c) in SHAPES.items():
        rows = groups * k
        z = torch.randn((rows, c), device=dev, generator=g)
        sc = torch.rand(c, device=dev, generator=g) + 0.5
        sh = torch.randn(c, device=dev, generator=g) * 0.1
        w = torch.rand(rows, device=dev, generator=g)
        zb = rows * c * 4
        for mode in ("avg", "weighted_avg", "max", "max_and_avg"):
            cw = 2 * c if mode == "max_and_avg" else c
            arg = mode in ("max", "max_and_avg")
            fwd_bytes = zb + (rows * 4 if mode == "weighted_avg" else 0) + groups * cw * 4 + (groups * c * 4 if arg else 0)
            t = timed(lambda: M.bn_relu_pool(z, k, sc, sh, True, mode, w=w, want_argmax=arg), a.iters)
            res.append(dict(shape=name, kernel="bn_relu_pool", mode=mode, us=t * 1e6, bytes=fwd_bytes, tb_s=fwd_bytes / t / 1e12,
                            frac_hbm=fwd_bytes / t / HBM))
            out, am = M.bn_relu_pool(z, k, sc, sh, True, mode, w=w, want_argmax=arg)
            gout = torch.randn(out.shape, device=dev, generator=g)
            bwd_bytes = zb + groups * cw * 4 + (rows * 4 if mode == "weighted_avg" else 0) + (groups * c * 4 if arg else 0)
            t = timed(lambda: M.sa_pool_grad(gout, k, c, mode, w=w, argmax=am), a.iters)
            res.append(dict(shape=name, kernel="sa_pool_grad", mode=mode, us=t * 1e6, bytes=bwd_bytes, tb_s=bwd_bytes / t / 1e12,
                            frac_hbm=bwd_bytes / t / HBM))
        mx_bytes = zb + 2 * groups * c * 4
        t = timed(lambda: M.bn_relu_max(z, k, sc, sh, True, want_argmax=True), a.iters)
        res.append(dict(shape=name, kernel="bn_relu_max", mode="max", us=t * 1e6, bytes=mx_bytes, tb_s=mx_bytes / t / 1e12,
                        frac_hbm=mx_bytes / t / HBM))
    for r in res:
        print("%-28s %-14s %-13s %9.2f us  %6.2f TB/s  %5.3f of HBM" % (r["shape"], r["kernel"], r["mode"], r["us"], r["tb_s"], r["frac_hbm"]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
