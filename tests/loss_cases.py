"""The cases of the loss kernel's tests, by id, each with its float64 reference (values, decisions, autograd cotangents) computed once
per process and shared by the tests that need it.  Test infrastructure: nothing here imports the package under test."""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref  # noqa: E402

NAMES = ["total_cost", "vote_reg_loss", "obj_cls_loss", "center_loss", "heading_cls_loss", "heading_residual_loss", "size_cls_loss",
         "size_residual_loss", "sem_cls_loss", "box_loss"]

# The smallest shapes that reach each branch of votenet_loss_kernel's role split (1024 threads = 16 waves; nbusy = min(ceil(P / 64), 16)
# waves own proposals, the other nfree take the boxes of the dual term and the seeds; P > 960: nfree = 0, the phases run in turn).
_D = dict(b=2, nh=12, ns=10, nc=10)
SHAPES = {
    "p1-all-minima": dict(b=2, n=1, p=1, bb=1, nh=1, ns=1, nc=1),       # softmax over one logit, N < nfree * 64
    "p63": dict(_D, n=70, p=63, bb=7),                                   # wave boundary of nbusy
    "p64": dict(_D, n=70, p=64, bb=7),
    "p65": dict(_D, n=70, p=65, bb=7),
    "p256-bb13": dict(_D, n=300, p=256, bb=13),                          # more boxes than the nfree = 12 waves
    "p256-bb40": dict(_D, n=300, p=256, bb=40),
    "p960-one-free-wave": dict(_D, n=130, p=960, bb=17),                 # nfree = 1: one wave takes every box and every seed
    "p961": dict(_D, n=130, p=961, bb=17),                               # not early, partial last wave
    "p1023": dict(_D, n=130, p=1023, bb=17),
    "p1024": dict(_D, n=130, p=1024, bb=17),
    "p1100-w229": dict(b=2, n=64, p=1100, bb=33, nh=32, ns=32, nc=32),   # two proposals per thread, the widest row
    "bb64": dict(_D, n=64, p=64, bb=64),                                 # box table beyond one wave of loaders
    "bb65": dict(_D, n=64, p=64, bb=65),
    "bb256": dict(_D, n=64, p=64, bb=256),                               # LOSS_MAXBOX
    "b9-n2049": dict(b=9, n=2049, p=128, bb=5, nh=12, ns=10, nc=10),     # scenes combined in order by the last workgroup
}


def case_ids():
    return ["shape-" + k for k in SHAPES] + ["hand-" + k for k in sorted(loss_ref.HAND_CASES)]


def label_case_ids():
    """The cases with one label at or past its range (loss_ref.LABEL_CASES); "labelbase-<base>" is the same case with every label valid."""
    return ["label-" + k for k in loss_ref.LABEL_CASES]


@functools.lru_cache(maxsize=None)
def label_box(cid):
    """-> (scene, box, field, the valid label the bad one replaced) of a "label-" case."""
    name = cid.split("-", 1)[1]
    _, (s, j), valid = loss_ref.label_case(name)
    return s, j, loss_ref.LABEL_CASES[name][0], valid


@functools.lru_cache(maxsize=None)
def load_case(cid):
    """-> seeds, votes, prop, out, gt, kw (nh / ns / nc / pos_thr / neg_thr as the reference and the kernel take them).  Shared: read-only."""
    kind, name = cid.split("-", 1)
    if kind in ("label", "labelbase"):
        case = loss_ref.label_case(name)[0] if kind == "label" else loss_ref.label_base(name)[0]
        kw = dict(nh=12, ns=10, nc=10)
    elif kind == "shape":
        s = SHAPES[name]
        case = loss_ref.shape_case(100 + list(SHAPES).index(name), **s)
        kw = dict(nh=s["nh"], ns=s["ns"], nc=s["nc"])
    else:
        case = loss_ref.HAND_CASES[name]()
        kw = dict(nh=12, ns=10, nc=10)
        if "thr" in loss_ref.HAND_EXPECT[name]:
            kw.update(pos_thr=loss_ref.HAND_EXPECT[name]["thr"][0], neg_thr=loss_ref.HAND_EXPECT[name]["thr"][1])
    for a in list(case[:4]) + list(case[4].values()):
        a.setflags(write=False)
    return case + (kw,)


@functools.lru_cache(maxsize=None)
def reference(cid):
    """float64: -> (dict of values, counts and decisions, dict of the cotangents of total_cost by autograd)."""
    seeds, votes, prop, out, gt, kw = load_case(cid)
    T = lambda a: torch.from_numpy(a.copy()).double() if a.dtype == np.float32 else torch.from_numpy(a.copy())
    v, p, w = T(votes).requires_grad_(True), T(prop).requires_grad_(True), T(out).requires_grad_(True)
    r = loss_ref.votenet_loss(T(seeds), v, p, w, {k: T(x) for k, x in gt.items()}, **kw)
    r["total_cost"].backward()
    r = {k: (x.detach() if isinstance(x, torch.Tensor) else x) for k, x in r.items()}
    return r, dict(votes_xyz=v.grad, proposals_xyz=p.grad, proposals_output=w.grad)
