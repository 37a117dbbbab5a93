"""GPU: the fused loss kernel (votenet_loss, csrc/loss.hip) against the numpy oracle of model.py:61-84,141-231 (values) and
against torch float64 autograd of the independent restatement (cotangents)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ["total_cost", "vote_reg_loss", "obj_cls_loss", "center_loss", "heading_cls_loss", "heading_residual_loss", "size_cls_loss",
         "size_residual_loss", "sem_cls_loss", "box_loss"]


def run_device(dev, seeds, votes, prop, out, gt):
    from votenet_amd import loss as VL
    o = dict(seeds_xyz=torch.from_numpy(seeds).to(dev), votes_xyz=torch.from_numpy(votes).to(dev),
             proposals_xyz=torch.from_numpy(prop).to(dev), proposals_output=torch.from_numpy(out).to(dev))
    return VL.votenet_loss(o, VL.gt_to_device(gt, dev))


@pytest.mark.parametrize("seed,shape", [(0, {}), (1, {}), (2, dict(b=8, n=1024, p=256, bb=9)), (3, dict(b=1, n=100, p=33, bb=1)),
                                        (4, dict(b=3, n=64, p=16, bb=16))])
def test_loss_values_and_cotangents(hiplib, dev, seed, shape):
    from oracle import oracle_loss
    seeds, votes, prop, out, gt = loss_ref.random_case(seed, **shape)
    losses, cot = run_device(dev, seeds, votes, prop, out, gt)
    got = dict(zip(NAMES + ["n_pos", "n_neg"], losses.cpu().tolist()))
    o = oracle_loss.votenet_loss(seeds, votes, prop, out, gt)
    assert int(got["n_pos"]) == o["n_pos"] > 0 and int(got["n_neg"]) == o["n_neg"] > 0
    for k in NAMES:
        assert abs(got[k] - float(o[k])) <= 1e-5 * max(1.0, abs(float(o[k]))), (k, got[k], float(o[k]))
    # cotangents: autograd of the float64 restatement
    T = lambda a: torch.from_numpy(a).double() if a.dtype == np.float32 else torch.from_numpy(a)
    v, p, w = T(votes).requires_grad_(True), T(prop).requires_grad_(True), T(out).requires_grad_(True)
    t = loss_ref.votenet_loss(T(seeds), v, p, w, {k: T(x) for k, x in gt.items()})
    t["total_cost"].backward()
    for name, ref in (("votes_xyz", v.grad), ("proposals_xyz", p.grad), ("proposals_output", w.grad)):
        g = cot[name].double().cpu()
        assert float((g - ref).abs().max()) <= 1e-5 * max(1e-3, float(ref.abs().max())), name
    # reproducible bit for bit (fixed-order reductions)
    losses2, _ = run_device(dev, seeds, votes, prop, out, gt)
    assert torch.equal(losses, losses2)


def test_loss_reads_a_column_slice_in_place(hiplib, dev):
    """votenet_loss_pitched: proposals_output as the first 79 columns of a wider row-major tensor (what the proposal module's last GEMM
    leaves) gives the losses and cotangents of the contiguous copy, bit for bit; the cotangent stays dense."""
    from votenet_amd import loss as VL
    seeds, votes, prop, out, gt = loss_ref.random_case(5, b=4, n=256, p=64, bb=7)
    ref_l, ref_c = run_device(dev, seeds, votes, prop, out, gt)
    wide = torch.full((out.shape[0], out.shape[1], 128), 1e30, device=dev)
    wide[:, :, :out.shape[2]] = torch.from_numpy(out).to(dev)
    o = dict(seeds_xyz=torch.from_numpy(seeds).to(dev), votes_xyz=torch.from_numpy(votes).to(dev),
             proposals_xyz=torch.from_numpy(prop).to(dev), proposals_output=wide[:, :, :out.shape[2]])
    assert not o["proposals_output"].is_contiguous()
    got_l, got_c = VL.votenet_loss(o, VL.gt_to_device(gt, dev))
    assert torch.equal(got_l, ref_l)
    for k in ref_c:
        assert torch.equal(got_c[k], ref_c[k]) and got_c[k].is_contiguous(), k


def test_loss_without_positives_is_nan_like_tensorflow(hiplib, dev):
    seeds, votes, prop, out, gt = loss_ref.random_case(7)
    losses, cot = run_device(dev, seeds, votes, (prop + 100.0).astype(np.float32), out, gt)
    l = losses.cpu().numpy()
    assert l[10] == 0 and np.isnan(l[0]) and np.isfinite(l[1])  # vote loss unaffected
    assert torch.isfinite(cot["proposals_output"]).all() and torch.isfinite(cot["votes_xyz"]).all()


def test_train_step_with_the_loss_graph(hiplib, dev):
    """config 3 in miniature: forward -> loss kernel -> backward -> Adam with the ground truth of the synthetic scenes; the
    total cost goes down over a few steps on one fixed batch."""
    from votenet_amd import loss as VL
    from votenet_amd import model as VM
    from votenet_amd import synth
    x = torch.from_numpy(synth.room_batch(4, 8192, 300)).to(dev)
    gt = VL.gt_to_device(synth.room_gt(4, 8192, 300), dev)
    net = VM.VoteNetHotPath(dev, seed=1)
    net.init_optimizer(1e-3)
    costs, npos = [], []
    for _ in range(16):
        net.train_step(x, gt=gt)
        l = net.last_losses.cpu().numpy()
        costs.append(float(l[0]))
        npos.append(int(l[10]))
    costs = np.array(costs)
    # a step without any positive proposal has a NaN cost (tf.reduce_mean of an empty tensor) and still finite parameters
    assert np.isfinite(costs[np.array(npos) > 0]).all() and np.isnan(costs[np.array(npos) == 0]).all()
    fin = costs[np.isfinite(costs)]
    assert len(fin) >= 8 and fin[-3:].mean() < fin[:3].mean()
    assert torch.isfinite(net.store.flat).all()


def test_decode_boxes_vs_oracle(hiplib, dev):
    """votenet_decode_boxes against the numpy restatement of model.py:100-129, and its corner order against what NMS3D
    expects (first four corners = top face, [0] / [4] span the height)."""
    from oracle import oracle_loss
    from votenet_amd import loss as VL
    from votenet_amd import synth
    rng = np.random.default_rng(11)
    prop = (rng.random((3, 50, 3)) * 4).astype(np.float32)
    out = rng.normal(0, 1.0, (3, 50, 79)).astype(np.float32)
    out[0, 0, 5 + 24 + 10:5 + 24 + 40] = -5.0  # residual below -1: the 1e-6 floor of model.py:119
    boxes, scores = VL.decode_boxes(torch.from_numpy(prop).to(dev), torch.from_numpy(out).to(dev))
    eb, es = oracle_loss.decode_boxes(prop, out, synth.MEAN_SIZES.astype(np.float32))
    assert np.abs(boxes.cpu().numpy() - eb).max() <= 1e-5 * max(1.0, np.abs(eb).max())
    assert (scores.cpu().numpy() == es).all()
    b = boxes.cpu().numpy()
    assert np.allclose(b[:, :, :4, 1], b[:, :, :1, 1], atol=1e-6) and (b[:, :, 0, 1] >= b[:, :, 4, 1]).all()


# ---------------------------------------------------------------- every role split, tie and threshold edge of votenet_loss_kernel
from loss_cases import case_ids, load_case, reference  # noqa: E402


def _to_dev(a, dev):
    return torch.from_numpy(a.copy()).to(dev)


def run_case(dev, cid, wide=0):
    """The case on the device: through loss.votenet_loss, or, where the case brings thresholds of its own, through the C ABI the way
    loss.py calls it.  wide: proposals_output as the first columns of a tensor that many columns wide (the pitched entry)."""
    from votenet_amd import _lib as L
    from votenet_amd import loss as VL
    seeds, votes, prop, out, gt, kw = load_case(cid)
    g = VL.gt_to_device({k: x.copy() for k, x in gt.items()}, dev)
    pout = _to_dev(out, dev)
    if wide:
        buf = torch.full(out.shape[:2] + (wide,), 1e30, device=dev)
        buf[:, :, :out.shape[2]] = pout
        pout = buf[:, :, :out.shape[2]]
        assert not pout.is_contiguous()
    o = dict(seeds_xyz=_to_dev(seeds, dev), votes_xyz=_to_dev(votes, dev), proposals_xyz=_to_dev(prop, dev), proposals_output=pout)
    if "pos_thr" not in kw:
        return VL.votenet_loss(o, g, nh=kw["nh"], ns=kw["ns"], nc=kw["nc"])
    assert not wide
    b, n, p, bb = seeds.shape[0], seeds.shape[1], prop.shape[1], gt["bboxes_xyz"].shape[1]
    losses = torch.empty(12, dtype=torch.float32, device=dev)
    cot = dict(votes_xyz=torch.zeros_like(o["votes_xyz"]), proposals_xyz=torch.zeros_like(o["proposals_xyz"]),
               proposals_output=torch.zeros_like(pout))
    ws = torch.zeros(int(L.lib().votenet_loss_workspace_floats(b)), dtype=torch.float32, device=dev)
    L.check(L.lib().votenet_loss_pitched(b, n, p, bb, kw["nh"], kw["ns"], kw["nc"], L.ptr(o["seeds_xyz"]), L.ptr(o["votes_xyz"]),
                                         L.ptr(o["proposals_xyz"]), L.ptr(pout), pout.stride(1), L.ptr(g["bboxes_xyz"]),
                                         L.ptr(g["bboxes_lwh"]), L.ptr(g["bboxes_roty"]), L.ptr(g["semantic_labels"]),
                                         L.ptr(g["heading_labels"]), L.ptr(g["heading_residuals"]), L.ptr(g["size_labels"]),
                                         L.ptr(g["size_residuals"]), kw["pos_thr"], kw["neg_thr"], L.ptr(losses), L.ptr(cot["votes_xyz"]),
                                         L.ptr(cot["proposals_xyz"]), L.ptr(cot["proposals_output"]), L.ptr(ws), L.stream_ptr()))
    return losses, cot


@pytest.mark.parametrize("cid", case_ids())
def test_loss_role_splits_ties_and_thresholds(hiplib, dev, cid):
    """The assertions of test_loss_values_and_cotangents (values and autograd cotangents of the float64 restatement at 1e-5 relative,
    floors 1.0 and 1e-3; a second run bit-identical) at every shape where votenet_loss_kernel splits its waves differently
    (loss_cases.SHAPES) and on the hand-made decisions (loss_ref.HAND_CASES), plus: a cotangent element whose float64 gradient is exactly
    zero (dead zone, seed outside every box, residual slot of another class, the loser of a tie) is bit-zero on the device.
    Measured on an MI355X: profiles/r07_loss_case_errors.txt."""
    losses, cot = run_case(dev, cid)
    r, g = reference(cid)
    got = dict(zip(NAMES + ["n_pos", "n_neg"], losses.cpu().tolist()))
    verr = {k: abs(got[k] - float(r[k])) / max(1.0, abs(float(r[k]))) for k in NAMES}
    cerr, stray = {}, {}
    for name, ref in g.items():
        d = cot[name].cpu()
        cerr[name] = float((d.double() - ref).abs().max()) / max(1e-3, float(ref.abs().max()))
        stray[name] = int((d.contiguous().view(torch.int32)[ref == 0] != 0).sum())
    print("loss_case %s n_pos=%d/%d n_neg=%d/%d value=%.2e (%s) votes_xyz=%.2e proposals_xyz=%.2e proposals_output=%.2e nonzero_where_ref_zero=%d"
          % (cid, got["n_pos"], r["n_pos"], got["n_neg"], r["n_neg"], max(verr.values()), max(verr, key=verr.get), cerr["votes_xyz"],
             cerr["proposals_xyz"], cerr["proposals_output"], sum(stray.values())))
    assert int(got["n_pos"]) == r["n_pos"] > 0 and int(got["n_neg"]) == r["n_neg"] > 0
    for k in NAMES:
        assert verr[k] <= 1e-5, (k, got[k], float(r[k]))
    for name in g:
        assert cerr[name] <= 1e-5, (name, cerr[name])
        assert stray[name] == 0, name
    losses2, cot2 = run_case(dev, cid)
    assert torch.equal(losses, losses2)
    for name in g:
        assert torch.equal(cot[name], cot2[name]), name


def test_loss_pitched_entry_on_the_not_early_path(hiplib, dev):
    """P = 961 (every wave owns proposals): the column slice of a wider tensor gives the contiguous copy's result bit for bit."""
    ref_l, ref_c = run_case(dev, "shape-p961")
    got_l, got_c = run_case(dev, "shape-p961", wide=128)
    assert torch.equal(got_l, ref_l)
    for k in ref_c:
        assert torch.equal(got_c[k], ref_c[k]) and got_c[k].is_contiguous(), k


def test_loss_rejects_shapes_beyond_its_tables(hiplib, dev):
    """257 boxes (LOSS_MAXBOX = 256) and nh = 33 (LOSS_MAXC = 32) raise before any launch, and the next valid call is unaffected."""
    from votenet_amd import InvalidArgumentError
    from votenet_amd import loss as VL
    before_l, before_c = run_case(dev, "shape-p63")
    for shape in (dict(bb=257), dict(nh=33)):
        seeds, votes, prop, out, gt = loss_ref.random_case(8, b=2, n=16, p=16, **shape)
        o = dict(seeds_xyz=_to_dev(seeds, dev), votes_xyz=_to_dev(votes, dev), proposals_xyz=_to_dev(prop, dev),
                 proposals_output=_to_dev(out, dev))
        with pytest.raises(InvalidArgumentError):
            VL.votenet_loss(o, VL.gt_to_device(gt, dev), nh=shape.get("nh", 12))
    after_l, after_c = run_case(dev, "shape-p63")
    assert torch.equal(before_l, after_l)
    for k in before_c:
        assert torch.equal(before_c[k], after_c[k]), k


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_loss_nonfinite_proposals_stay_inside_the_buffers(hiplib, dev, bad):
    """A diverged run: every proposal centre of scene 0 is NaN (or +inf), scene 1 is ordinary.  No proposal is then at a distance below
    infinity from any box, and the dual term's arg-min keeps its sentinel index: it used to be turned into an address.  It falls back to
    proposal 0, as tf.argmin over all-NaN / all-inf distances: total_cost and center_loss are NaN for NaN centres (+inf for +inf centres:
    Huber of an infinite error is +inf and nothing turns it into NaN, in the float64 restatement as on the device), the vote loss and the
    votes' cotangents are those of the run with scene 0 finite, bit for bit, and guard bands around the output buffers are untouched."""
    from votenet_amd import _lib as L
    from votenet_amd import loss as VL
    seeds, votes, prop, out, gt = loss_ref.random_case(9, b=2, n=64, p=70, bb=6)
    g = VL.gt_to_device(gt, dev)
    o = dict(seeds_xyz=_to_dev(seeds, dev), votes_xyz=_to_dev(votes, dev), proposals_xyz=_to_dev(prop, dev), proposals_output=_to_dev(out, dev))
    fin_l, fin_c = VL.votenet_loss(o, g)
    broken = prop.copy()
    broken[0] = bad
    o["proposals_xyz"] = _to_dev(broken, dev)
    GUARD, SENTINEL = 1024, -7777.0
    need = votes.size + prop.size + out.size + int(L.lib().votenet_loss_workspace_floats(2))
    big = torch.full((GUARD + need + GUARD,), SENTINEL, device=dev)
    bigl = torch.full((GUARD + 12 + GUARD,), SENTINEL, device=dev)
    flat, losses = big[GUARD:GUARD + need], bigl[GUARD:GUARD + 12]
    flat.zero_()
    got_l, got_c = VL.votenet_loss(o, g, buffers=(losses, flat))
    torch.cuda.synchronize()
    assert got_l.data_ptr() == losses.data_ptr() and got_c["votes_xyz"].data_ptr() == flat.data_ptr()
    for t, n in ((big, need), (bigl, 12)):
        assert (t[:GUARD] == SENTINEL).all() and (t[GUARD + n:] == SENTINEL).all()
    l, f = got_l.cpu().numpy(), fin_l.cpu().numpy()
    T = lambda a: torch.from_numpy(a).double() if a.dtype == np.float32 else torch.from_numpy(a)
    r = loss_ref.votenet_loss(T(seeds), T(votes), T(broken), T(out), {k: T(x) for k, x in gt.items()})
    want = np.nan if np.isnan(bad) else np.inf
    for k in ("total_cost", "center_loss"):
        assert np.array_equal(float(r[k]), want, equal_nan=True) and np.array_equal(l[NAMES.index(k)], want, equal_nan=True), (k, l)
    assert (l[10], l[11]) == (r["n_pos"], r["n_neg"]) and r["n_pos"] > 0
    for i, k in enumerate(NAMES):  # the terms the broken scene cannot reach keep the bar of the other tests
        if np.isfinite(float(r[k])):
            assert abs(l[i] - float(r[k])) <= 1e-5 * max(1.0, abs(float(r[k]))), (k, l[i], float(r[k]))
    assert np.isfinite(l[1]) and l[1] == f[1]
    assert torch.equal(got_c["votes_xyz"], fin_c["votes_xyz"]) and bool((got_c["votes_xyz"][1] != 0).any())


@pytest.mark.parametrize("b,p,nh", [(3, 85, 12), (2, 128, 12), (1, 257, 12), (1, 257, 1)])
def test_decode_boxes_hand_cases(hiplib, dev, b, p, nh):
    """decode_boxes_kernel where a draw of Gaussians never goes: 2 * bin + residual below zero, at 2 * nh exactly and above it (both sides
    of floormod), a size residual of -1 and below (the 1e-6 floor), exact ties in the heading and the size arg-max (the first wins: the
    tied bins carry different residuals), nh = 1, and b * P = 255, 256, 257 proposals on blocks of 256 (the cases sit in the first rows
    and again in the last one).  Bar: that of test_decode_boxes_vs_oracle."""
    from oracle import oracle_loss
    from votenet_amd import loss as VL
    from votenet_amd import synth
    rng = np.random.default_rng(12)
    ns, nc = 10, 10
    W, so = 5 + 2 * nh + 4 * ns + nc, 5 + 2 * nh
    prop = (rng.random((b, p, 3)) * 4).astype(np.float32)
    out = rng.normal(0, 1.0, (b, p, W)).astype(np.float32)
    rows, hb = out.reshape(-1, W), nh - 1

    def heading(r, bins, residuals):
        r[5:5 + nh] = -4.0
        for i, res in zip(bins, residuals):
            r[5 + i], r[5 + nh + i] = 2.0, res

    def size(r, classes, residuals):
        r[so:so + ns] = -4.0
        for i, res in zip(classes, residuals):
            r[so + i] = 2.0
            r[so + ns + 3 * i:so + ns + 3 * i + 3] = res

    heading(rows[0], [0], [-0.5])                   # negative
    heading(rows[1], [hb], [2.5])                   # 2 (nh - 1) + 2.5 >= 2 nh
    heading(rows[2], [hb], [2.0])                   # 2 nh exactly
    heading(rows[3], [hb, 0], [0.25, -30.0])        # tie: bin 0 wins, far below zero
    size(rows[4], [3, 6], [(0.5, -0.25, 0.125), (-0.5, 2.0, 1.0)])   # tie: class 3 wins
    size(rows[5], [7], [(-1.0, -1.0, 0.0)])         # 1 + residual = 0: the floor
    size(rows[6], [9, 2], [(-3.5, 0.5, -1.0 - 2.0 ** -20), (0.0, 0.0, 0.0)])  # tie: class 2 wins, although class 9 was written first
    heading(rows[-1], [hb, 0], [3.0, -0.5])
    size(rows[-1], [8, 4], [(0.0, 0.0, 0.0), (-1.5, 0.25, -1.0)])
    boxes, scores = VL.decode_boxes(_to_dev(prop, dev), _to_dev(out, dev), nh=nh)
    eb, es = oracle_loss.decode_boxes(prop, out, synth.MEAN_SIZES.astype(np.float32), nh=nh)
    got = boxes.cpu().numpy()
    assert got.shape == (b, p, 8, 3)
    assert np.abs(got - eb).max() <= 1e-5 * max(1.0, np.abs(eb).max())
    assert (scores.cpu().numpy() == es).all()
    flat = got.reshape(-1, 8, 3)
    extent = lambda q: flat[q].max(0) - flat[q].min(0)
    assert extent(5)[1] > 0.1 and np.hypot(extent(5)[0], extent(5)[2]) < 1e-5    # l and w on the floor, h untouched
    # the first of a tie, told by its residuals: class 4 of the last row has h on the floor, class 8 would not
    assert extent(-1)[1] < 1e-5 and extent(4)[1] == pytest.approx(synth.MEAN_SIZES[3][2] * 1.125, rel=1e-5)


# ---------------------------------------------------------------- labels at or past their range (loss_ref.LABEL_CASES)
import functools  # noqa: E402

from loss_cases import label_box, label_case_ids  # noqa: E402

LABEL_GUARD = 4096          # elements of sentinel on both sides of every buffer: more than the widest index a label of these cases could make (column 3071)
F_SENTINEL, I_SENTINEL = -7777.0, 0x5A5A5A5A


def _inside_sentinels(a, dev, zero=False):
    """A buffer with the contents of `a` (or zeros of its shape) in the middle of a sentinel-filled tensor -> (whole tensor, view)."""
    t = torch.from_numpy(np.array(a))  # (a copy: the shared cases are read-only)
    big = torch.full((LABEL_GUARD + t.numel() + LABEL_GUARD,), I_SENTINEL if t.dtype == torch.int32 else F_SENTINEL, dtype=t.dtype, device=dev)
    view = big[LABEL_GUARD:LABEL_GUARD + t.numel()].view(t.shape)
    if zero:
        view.zero_()
    else:
        view.copy_(t.to(dev))
    return big, view


def _margins_intact(big, n):
    fill = I_SENTINEL if big.dtype == torch.int32 else F_SENTINEL
    return bool((big[:LABEL_GUARD] == fill).all()) and bool((big[LABEL_GUARD + n:] == fill).all())


def run_case_inside_sentinels(dev, cid):
    """The case through the C ABI with every input and every output carved out of a sentinel-filled tensor of its own.  Asserts that no
    margin was written and no input changed; -> (losses, cotangents) as CPU tensors."""
    from votenet_amd import _lib as L
    seeds, votes, prop, out, gt, kw = load_case(cid)
    b, n, p, bb = seeds.shape[0], seeds.shape[1], prop.shape[1], gt["bboxes_xyz"].shape[1]
    GT = ("bboxes_xyz", "bboxes_lwh", "bboxes_roty", "semantic_labels", "heading_labels", "heading_residuals", "size_labels", "size_residuals")
    host = dict(seeds=seeds, votes=votes, prop=prop, out=out, **{k: gt[k] for k in GT})
    ins = {k: _inside_sentinels(a, dev) for k, a in host.items()}
    nws = int(L.lib().votenet_loss_workspace_floats(b))
    outs = dict(losses=_inside_sentinels(np.zeros(12, np.float32), dev, zero=True), d_votes=_inside_sentinels(votes, dev, zero=True),
                d_prop=_inside_sentinels(prop, dev, zero=True), d_out=_inside_sentinels(out, dev, zero=True),
                ws=_inside_sentinels(np.zeros(nws, np.float32), dev, zero=True))
    P = lambda k: L.ptr((ins[k] if k in ins else outs[k])[1])
    L.check(L.lib().votenet_loss(b, n, p, bb, kw["nh"], kw["ns"], kw["nc"], P("seeds"), P("votes"), P("prop"), P("out"), P("bboxes_xyz"),
                                 P("bboxes_lwh"), P("bboxes_roty"), P("semantic_labels"), P("heading_labels"), P("heading_residuals"),
                                 P("size_labels"), P("size_residuals"), 0.3, 0.6, P("losses"), P("d_votes"), P("d_prop"), P("d_out"),
                                 P("ws"), L.stream_ptr()))
    torch.cuda.synchronize()
    for k, (big, view) in list(ins.items()) + list(outs.items()):
        assert _margins_intact(big, view.numel()), "the margin of %s was written" % k
    for k, (big, view) in ins.items():
        assert np.array_equal(view.cpu().numpy(), host[k]), "input %s was written" % k
    return outs["losses"][1].cpu(), dict(votes_xyz=outs["d_votes"][1].cpu(), proposals_xyz=outs["d_prop"][1].cpu(),
                                         proposals_output=outs["d_out"][1].cpu())


@functools.lru_cache(maxsize=None)
def _valid_label_run(dev, base):
    return run_case_inside_sentinels(dev, "labelbase-" + base)


def _i32(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("cid", label_case_ids())
def test_loss_label_outside_its_range(hiplib, dev, cid):
    """One ground-truth box carries one label at or past its range (heading nh / -1, size ns / -1 / ns + 1000, semantic nc / -1); positives
    are assigned to it, the last row of the buffers among them.  Defined behaviour (include/votenet_hip.h, tests/loss_ref.py): the class
    term is NaN and the class block of those proposals' cotangent rows is NaN; the residual prediction is 0 (an all-zero one-hot row):
    Huber(0 - label residual) in the loss, no cotangent.  Checked here:
    - every input and output lies between 4096-element sentinel margins, none of which changes, and no input changes;
    - NaN exactly where the float64 reference has NaN; everything finite at the bar of the other tests (1e-5 relative, floors 1.0 and
      1e-3), bit-zero where the reference is exactly zero;
    - against the device's own run with the valid label: the loss terms the label does not enter, the votes' and proposal centres'
      cotangents, and every entry of proposals_output's cotangent outside the class block and the valid label's residual slot of the
      mislabelled box's positives keep every bit."""
    losses, cot = run_case_inside_sentinels(dev, cid)
    s, j, field, valid = label_box(cid)
    base = loss_ref.LABEL_CASES[cid.split("-", 1)[1]][2]
    losses0, cot0 = _valid_label_run(dev, base)
    r, g = reference(cid)
    r0, g0 = reference("labelbase-" + base)
    got, got0 = dict(zip(NAMES + ["n_pos", "n_neg"], losses.tolist())), dict(zip(NAMES + ["n_pos", "n_neg"], losses0.tolist()))
    print("label_case %s box (%d, %d) valid label %d losses %s" % (cid, s, j, valid, got))
    assert int(got["n_pos"]) == r["n_pos"] > 0 and int(got["n_neg"]) == r["n_neg"] > 0
    for i, k in enumerate(NAMES):
        want = float(r[k])
        if np.isnan(want):
            assert k in loss_ref.LABEL_NAN[field] and np.isnan(got[k]), (k, got[k])
        else:
            assert abs(got[k] - want) <= 1e-5 * max(1.0, abs(want)), (k, got[k], want)
        if k not in loss_ref.LABEL_AFFECTS[field]:
            assert torch.equal(_i32(losses[i:i + 1]), _i32(losses0[i:i + 1])), (k, got[k], got0[k])
        assert abs(got0[k] - float(r0[k])) <= 1e-5 * max(1.0, abs(float(r0[k]))), (k, got0[k], float(r0[k]))  # the valid run is a valid run
    for name, ref in g.items():
        d = cot[name]
        nan = torch.isnan(ref)
        assert torch.equal(torch.isnan(d), nan), name
        fin = ~nan
        err = float((d.double()[fin] - ref[fin]).abs().max()) / max(1e-3, float(ref[fin].abs().max()))
        print("label_case %s %s error %.2e NaN entries %d" % (cid, name, err, int(nan.sum())))
        assert err <= 1e-5, (name, err)
        assert int((_i32(d)[ref == 0] != 0).sum()) == 0, name
    assert torch.equal(_i32(cot["votes_xyz"]), _i32(cot0["votes_xyz"])) and torch.equal(_i32(cot["proposals_xyz"]), _i32(cot0["proposals_xyz"]))
    mine = (r["positive"][s] & (r["bboxes_assignment"][s] == j)).numpy()
    cls_cols, res_cols = loss_ref.label_blocks(field, valid)
    may_differ = np.zeros(cot["proposals_output"].shape, bool)
    may_differ[s][np.ix_(mine, list(cls_cols) + list(res_cols))] = True
    a, a0 = _i32(cot["proposals_output"]).numpy(), _i32(cot0["proposals_output"]).numpy()
    assert mine.sum() >= 2 and mine[-1] and s == a.shape[0] - 1
    assert np.array_equal(a[~may_differ], a0[~may_differ])
    assert np.isnan(cot["proposals_output"].numpy()[s][np.ix_(mine, list(cls_cols))]).all()
    if res_cols:
        assert (a[s][np.ix_(mine, res_cols)] == 0).all() and (a0[s][np.ix_(mine, res_cols)] != 0).all()
