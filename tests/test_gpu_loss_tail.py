"""GPU: what runs behind the loss launch and the pieces it shares.  VoteNetHotPath._after_loss is the one place a train step -- launch
path, eager first step of a shape, replayed graphs -- issues the paper vote launch, the paper proposal launch and the monitors' accuracy
launch from: last_accuracies must be the same object with the same bits on all three paths.  csrc/scene_fold.h is the one text of the
per-scene fold at the end of paper_vote_loss_kernel and paper_proposal_loss_kernel: a case whose result depends on the ORDER in which
the scenes' sums are added.  _lib.dev_f32_rows is the one test for rows read in place."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F = np.float32
B, NPTS, SMALL = 2, 4096, (512, 256, 128, 64)  # the suite's small training shape (test_gpu_monitors.py)


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _batch(dev, seed):
    from votenet_amd import loss as VL
    from votenet_amd import synth
    return torch.from_numpy(synth.room_batch(B, NPTS, seed)).to(dev), VL.gt_to_device(synth.room_gt(B, NPTS, seed), dev)


def _monitored_net(dev, seed):
    from votenet_amd import model as VM
    net = VM.VoteNetHotPath(dev, seed=seed, npoints=SMALL)
    net.init_optimizer(1e-3)
    net.enable_monitors(window=8)
    return net


def _step_and_check(net, x, gt, path):
    """One step; last_accuracies is the monitors' tensor and holds votenet_accuracies of THIS step's forward results, bit for bit."""
    from votenet_amd import loss as VL
    out = net.train_step(x, gt=gt)
    step_out = {k: out[k].clone() for k in ("proposals_xyz", "proposals_output")}  # before the next replay rewrites them
    assert net.last_accuracies is net.monitors.accuracies, path
    got = bits(net.last_accuracies)
    want, _ = VL.votenet_accuracies(step_out, gt)
    print(path, "accuracies", net.last_accuracies.tolist(), "recomputed", want.tolist())
    assert torch.equal(got, bits(want)), path


def test_last_accuracies_on_the_deterministic_launch_path(hiplib, dev):
    from votenet_amd import mlp as M
    x, gt = _batch(dev, 470)
    prev = M.set_deterministic(True)
    try:
        net = _monitored_net(dev, 12)
        _step_and_check(net, x, gt, "launch path")
        assert not net.__dict__.get("_stretch_graphs")
    finally:
        M.set_deterministic(prev)


def test_last_accuracies_on_the_first_step_of_a_shape_and_on_a_replayed_step(hiplib, dev):
    from votenet_amd import mlp as M
    from votenet_amd import model as VM
    assert not M.DETERMINISTIC and VM.STRETCH_GRAPH
    net = _monitored_net(dev, 13)
    replays = []
    for seed, path in ((472, "eager first step"), (474, "captured and replayed"), (476, "replayed")):
        x, gt = _batch(dev, seed)
        _step_and_check(net, x, gt, path)
        replays.append(sum(g.replays for g in net.__dict__.get("_stretch_graphs", {}).values()))
    assert replays[0] == 0 and replays[2] > replays[1] >= 1, "the steps did not take the paths they are named for: %s" % replays
    assert net.monitors.steps == 3


@pytest.mark.parametrize("big", [0, 8], ids=["big-scene-first", "big-scene-last"])
def test_the_scenes_sums_are_folded_in_scene_order(hiplib, dev, big):
    """paper_vote_loss has one sum per scene.  Nine scenes of 64 seeds, one box each (a cube of side 2 at the origin): in scene `big` all
    seeds sit at the origin and every vote is (2^18, 0, 0), a sum of exactly 2^24; in each of the other eight, seed 0 sits at the origin
    with the vote (1, 0, 0) and the others lie outside, a sum of exactly 1.  Every scene's sum is exact in fp32, so only the order across
    the scenes decides the result: with the big scene first every + 1 is lost in turn, with the big scene last all eight count."""
    from votenet_amd import vote_supervision as VS
    b, n = 9, 64
    seeds = np.full((b, n, 3), 10.0, F)
    seeds[:, 0] = 0.0
    seeds[big] = 0.0
    votes = np.zeros((b, n, 3), F)
    votes[:, 0, 0] = 1.0
    votes[big, :, 0] = 2.0 ** 18
    gt = dict(bboxes_xyz=np.zeros((b, 1, 3), F), bboxes_lwh=np.full((b, 1, 3), 2.0, F), bboxes_roty=np.zeros((b, 1), F))
    T = lambda a: torch.from_numpy(a).to(dev)
    out, g = dict(seeds_xyz=T(seeds), votes_xyz=T(votes)), {k: T(v) for k, v in gt.items()}
    inv = F(1) / (F(72) + F(1e-6))
    first, last = F(2.0 ** 24) * inv, F(2.0 ** 24 + 8) * inv
    assert first != last and F(2.0 ** 24) + F(1) == F(2.0 ** 24) and float(F(2.0 ** 24 + 8)) == 2.0 ** 24 + 8
    want = first if big == 0 else last
    l0 = np.random.default_rng(3).random(12).astype(F) + F(0.25)
    work = VS.workspace(b, dev)
    for run in range(2):  # twice over one workspace: the launch leaves it zero
        losses = T(l0.copy())
        _, sup = VS.paper_vote_loss(out, g, losses, work=work)
        l = losses.cpu().numpy()
        print("big scene at", big, "run", run, "P", int(sup), "vote_reg_loss", float(l[1]), "expected", float(want), "other order",
              float(last if big == 0 else first))
        assert int(sup) == 72
        assert l[1:2].view(np.int32)[0] == np.array([want], F).view(np.int32)[0]
        assert not work.any()


def test_rows_with_unit_column_stride_are_read_in_place(hiplib, dev):
    from votenet_amd import _lib as L
    wide = torch.arange(2 * 8 * 96, dtype=torch.float32, device=dev).reshape(2, 8, 96)
    view = wide[:, :, 5:84]
    assert tuple(view.shape) == (2, 8, 79) and not view.is_contiguous()
    same = L.dev_f32_rows(view, "rows")
    assert same.data_ptr() == view.data_ptr() and same.stride() == (8 * 96, 96, 1) and tuple(same.shape) == (2, 8, 79)
    whole = L.dev_f32_rows(wide, "rows")
    assert whole.data_ptr() == wide.data_ptr() and whole.is_contiguous()
    every_other = wide[:, :, ::2]
    copy = L.dev_f32_rows(every_other, "rows")
    assert copy.is_contiguous() and copy.data_ptr() != every_other.data_ptr() and torch.equal(copy, every_other)
    uneven = wide[:, ::2, :79].transpose(0, 1)  # unit column stride, but no uniform pitch over the first two axes
    copy = L.dev_f32_rows(uneven, "rows")
    assert copy.is_contiguous() and torch.equal(copy, uneven)
    cpu = torch.zeros(2, 8, 79)
    with pytest.raises(L.VotenetError) as a:
        L.dev_f32(cpu, "rows", 3)
    with pytest.raises(L.VotenetError) as e:
        L.dev_f32_rows(cpu, "rows")
    assert type(e.value) is type(a.value) and str(e.value) == str(a.value) and "must live on the GPU" in str(e.value)
    with pytest.raises(L.InvalidArgumentError, match="rows expects rank 3"):
        L.dev_f32_rows(wide[0], "rows")
