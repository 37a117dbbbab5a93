"""GPU: the inference-mode forward pass -- VoteNetHotPath.predict's BatchNorm on the moving averages (inference_bn -> mlp.FrozenBN ->
pointnet2.frozen_bn) -- against tests/inference_ref.py, a float64 restatement of the stack on the device's own indices.  The frozen
mode takes branches the training-mode forward never does (the table entry in place of the launch's sums, finished scale / shift
vectors in every consumer, no first-layer statistics, no stored z behind the pool, the pooled extreme picked by the sign of gamma), and
nothing else compares them with a reference.

Shape: synth.room_batch(2, 2048), npoints (512, 256, 128, 64).  The moving statistics are written to differ from the batch's
(moving_mean = mean + 0.5 sqrt(var) randn, moving_var = var U(0.5, 2)), so a path that kept using batch sums misses the bar by orders
of magnitude (asserted on the two references).  Two parameter sets: `perturbed` (gamma = 1 + 0.2 randn, as test_gpu_model's) and
`signed` (gamma = 0.2 + 0.3 randn, every 7th channel exactly 0: negative and zero scales in every layer).

Bars (the project's own; error = max |got - ref| / max(1, max |ref|)):
  MODULE_BAR 2e-5   a module's output on the reference's input, and the chained seeds / votes (tests/test_gpu_model.py:69-78)
  STACK_BAR  5e-5   the end of the whole stack, proposals_output (tests/test_gpu_backward.py:127)
  bn_stats_ref.BAR  the moving averages, on the layer's normalised output
Every test prints what it measured."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inference_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

MODULE_BAR = 2e-5
STACK_BAR = 5e-5
NPOINTS = (512, 256, 128, 64)
SEED_X, SEED_NET = 77, 3
CHAINED = ("seeds_points", "votes_xyz", "votes_points")  # held to MODULE_BAR in a chained run; proposals_output to STACK_BAR
_CACHE = {}  # references and moving statistics: computed once, shared, never modified


# ------------------------------------------------------------------------------------------------------------------ set-up
def scenes(b=2):
    from votenet_amd import synth
    return synth.room_batch(b, 2048, SEED_X)  # (scene i is the same whatever b is)


def make_net(dev, gammas):
    """A net with the BatchNorm affine parameters and the biases perturbed as test_gpu_model._perturbed_net does; gammas "signed":
    gamma = 0.2 + 0.3 randn (the form of tests/test_gpu_half.py:122) with every 7th channel exactly 0."""
    from votenet_amd import model as VM
    net = VM.VoteNetHotPath(dev, seed=SEED_NET, npoints=NPOINTS)
    g = torch.Generator().manual_seed(1)
    for name, v in net.store.views.items():
        if name.endswith("gamma"):
            if gammas == "signed":
                t = 0.2 + 0.3 * torch.randn(v.shape, generator=g)
                t[::7] = 0.0
            else:
                t = 1 + 0.2 * torch.randn(v.shape, generator=g)
            v.copy_(t.to(dev))
        if name.endswith("beta") or name.endswith("/b"):
            v.copy_((0.1 * torch.randn(v.shape, generator=g)).to(dev))
    net.store.params_changed()
    assert [L.name for L in net._bn_layers()] and sorted(L.name for L in net._bn_layers()) == sorted(R.bn_layer_names())
    if gammas == "signed":  # a negative and a zero scale in every first layer and every pooled last layer
        for name in ["sa%d/conv%d" % (i, j) for i in (1, 2, 3, 4) for j in (0, 2)] + ["proposal/conv0", "proposal/conv2", "fp1/conv_0",
                                                                                     "fp2/conv_0", "voting/fc0", "proposal/conv_post_0"]:
            gm = net.store[name + "/gamma"]
            assert int((gm < 0).sum()) > 0 and int((gm == 0).sum()) > 0 and int((gm > 0).sum()) > 0, name
    return net


def params_of(net):
    return {k: v.detach().cpu().clone() for k, v in net.store.views.items()}


def tape_geometry(tape):
    """The indices a taped pass ran on: they depend on coordinates only (held to the oracle by tests/test_gpu_model.py)."""
    g = {"sa%d" % (i + 1): dict(fps_idx=tape[i]["fps_idx"].cpu(), idx=tape[i]["idx"].cpu()) for i in range(4)}
    for name, t in (("fp1", tape[4]), ("fp2", tape[5])):
        assert t["op"] == "fp"
        g[name] = dict(idx=t["idx"].cpu(), weight=t["weight"].cpu())
    g["proposal"] = None
    return g


def fresh_geometry(net, x):
    """The same indices from the project's geometry functions (a batch no taped pass has seen)."""
    from votenet_amd import pointnet2 as P
    g, xyz = {}, x
    for name in ("sa1", "sa2", "sa3", "sa4"):
        m = getattr(net, name)
        fps_idx, new_xyz, idx, _ = P.sample_and_group(m.npoint, m.radius, m.nsample, xyz)
        g[name] = dict(fps_idx=fps_idx.cpu(), idx=idx.cpu(), new_xyz=new_xyz)
        xyz = new_xyz
    for name, a, b in (("fp1", "sa3", "sa4"), ("fp2", "sa2", "sa3")):
        fg = P.FPModule.geometry(g[a]["new_xyz"], g[b]["new_xyz"])
        g[name] = dict(idx=fg.idx.cpu(), weight=fg.weight.cpu())
    g["proposal"] = None
    return g


def scene_of(g, s):
    """Scene s of a batch's geometry: every index is scene-local."""
    return {k: (None if v is None else {kk: vv[s:s + 1] for kk, vv in v.items() if kk != "new_xyz"}) for k, v in g.items()}


def proposal_geometry(net, votes_xyz, seeds_xyz):
    """The proposal module's grouping of THESE votes (it depends on their coordinates to the last bit): FPS on the seeds, centres
    gathered from the votes, ball query -- the project's own kernels, as test_forward_small_vs_oracle regroups with the oracle's."""
    from votenet_amd import pointnet2 as P
    pr = net.proposal
    fps_idx = P.tf_sampling.farthest_point_sample(pr.npoint, seeds_xyz)
    new_xyz = P.tf_sampling.gather_point(votes_xyz, fps_idx)
    idx, _ = P.tf_grouping.query_ball_point(pr.radius, pr.nsample, votes_xyz, new_xyz)
    return dict(fps_idx=fps_idx.cpu(), idx=idx.cpu()), new_xyz


def setup(dev, gammas):
    """-> dict(net, x, params, geometry, stats): a net of the parameter set with the moving statistics installed.  The statistics and the
    geometry are made once per parameter set (one training-mode forward pass with a tape) and reused: every later net of the set gets
    the same numbers."""
    net = make_net(dev, gammas)
    x = torch.from_numpy(scenes()).to(dev)
    key = ("setup", gammas)
    if key not in _CACHE:
        tape = []
        net.forward(x, tape)
        torch.cuda.synchronize()
        assert [t["op"] for t in tape] == ["sa"] * 4 + ["fp", "fp", "vote", "sa"]
        g = torch.Generator().manual_seed(2)
        stats = {}
        for r in net._bn_records(tape):
            mean, var = r["mean"].cpu().double(), r["var"].cpu().double()
            mm = mean + 0.5 * var.sqrt() * torch.randn(mean.shape, generator=g, dtype=torch.float64)
            mv = var * (0.5 + 1.5 * torch.rand(mean.shape, generator=g, dtype=torch.float64))
            stats[r["layer"].name] = (mm.float(), mv.float())
        assert sorted(stats) == sorted(R.bn_layer_names())
        _CACHE[key] = dict(params=params_of(net), geometry=tape_geometry(tape), stats=stats)
    c = _CACHE[key]
    install(net, c["stats"])
    return dict(net=net, x=x, gammas=gammas, **c)


def install(net, stats):
    """The moving statistics into the net's (4, c) blocks, and the version bump that makes inference_bn() rebuild its table (as
    step_guard.py and checkpoint.py do after they wrote the averages)."""
    ema = net._ema_state()
    assert sorted(ema) == sorted(stats) and len(ema) == 23
    for name, (mm, mv) in stats.items():
        ema[name][2].copy_(mm.to(net.device))
        ema[name][3].copy_(mv.to(net.device))
    net._ema_version += 1


def base_ref(s, mode, scene=None, geometry=None, x=None):
    """The reference up to the votes (shared by every run of this parameter set, mode and batch; the proposal module is added per run on
    a copy: propose)."""
    key = ("ref", s["gammas"], mode, scene)
    if key not in _CACHE:
        geo = geometry if geometry is not None else s["geometry"]
        xs = x if x is not None else s["x"]
        _CACHE[key] = R.forward_ref(s["params"], s["stats"], geo, xs.cpu(), mode)
    return _CACHE[key]


def propose(s, base, mode, pg):
    """(out, bn) of base completed with the proposal module on the grouping pg; base itself stays as it is."""
    out, bn = dict(base[0]), dict(base[1])
    R.propose_ref(s["params"], s["stats"], pg, out, mode, bn)
    return out, bn


def check_stack(s, got, base, mode, what, sl=slice(None)):
    """A chained run `got` (the dict forward / predict return; sl: the scenes of it that `base` covers) against the reference: seeds and
    votes to MODULE_BAR, proposals_xyz exact, proposals_output to STACK_BAR.  -> the measured errors."""
    net = s["net"]
    vx, sx = got["votes_xyz"][sl].contiguous(), got["seeds_xyz"][sl].contiguous()
    pg, new_xyz = proposal_geometry(net, vx, sx)
    assert torch.equal(got["proposals_xyz"][sl], new_xyz), what  # FPS on the seeds, centres gathered from the run's own votes
    ref, _ = propose(s, base, mode, pg)
    assert np.array_equal(got["seeds_xyz"][sl].cpu().double().numpy(), ref["seeds_xyz"].numpy()), what
    errs = {k: R.relerr(got[k][sl], ref[k]) for k in CHAINED + ("proposals_output",)}
    errs["proposals_xyz"] = R.relerr(got["proposals_xyz"][sl], ref["proposals_xyz"])
    print("MEASURED %s: %s" % (what, "  ".join("%s=%.2e" % kv for kv in errs.items())))
    for k in CHAINED + ("proposals_xyz",):
        assert errs[k] < MODULE_BAR, (what, k, errs)  # measured: <= 2.9e-6 in inference mode, <= 5.5e-6 in training mode (signed gammas)
    assert errs["proposals_output"] < STACK_BAR, (what, errs)  # measured: <= 6.3e-6 in inference mode, <= 2.6e-5 in training mode
    assert got["proposals_output"][sl].shape[1:] == (256, 79)
    return errs


def references_differ(s):
    """The two modes are different functions of this set-up by far more than any bar: a path that kept using batch sums cannot pass."""
    a, b = base_ref(s, "moving")[0], base_ref(s, "batch")[0]
    for k in CHAINED:
        assert R.relerr(a[k], b[k]) > 1000 * STACK_BAR, (k, R.relerr(a[k], b[k]))


def run_mode(s, mode, tape=None):
    """The device pass of `mode`: predict(x) -- untaped, moving averages -- or a plain training-mode forward."""
    from votenet_amd import pointnet2 as P
    net, x = s["net"], s["x"]
    if mode == "moving" and tape is None:
        out = net.predict(x)
    elif mode == "moving":
        with P.frozen_bn(net.inference_bn()):
            out = net.forward(x, tape)
    else:
        out = net.forward(x, tape)
    torch.cuda.synchronize()
    return out


CASES = [("perturbed", "moving"), ("signed", "moving"), ("signed", "batch")]  # (perturbed, batch) is test_gpu_model's, against the oracle
CASE_IDS = ["%s-%s" % c for c in CASES]
FORMS = {2: "fp16x2_forward_images", 1: "bf16x3_images", 0: "fp32_mfma"}


# ------------------------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("gammas,mode", CASES, ids=CASE_IDS)
def test_whole_stack_vs_float64(hiplib, dev, gemm_form, gammas, mode):
    """predict(x) -- tape None, moving averages -- against forward_ref(mode="moving"), and with signed gammas also the plain
    training-mode forward(x) against forward_ref(mode="batch"): the composed training forward has not met a negative gamma either.
    Measured on an MI355X, seeds_points / votes_xyz / votes_points / proposals_output, worst of the two moving-average cases | the
    signed training-mode case:
      fp16x2_forward_images  1.7e-6 / 2.6e-6 / 1.9e-6 / 5.2e-6  |  4.6e-6 / 1.2e-6 / 5.1e-6 / 2.1e-5
      bf16x3_images          2.8e-6 / 2.5e-6 / 2.9e-6 / 6.3e-6  |  5.5e-6 / 1.3e-6 / 5.5e-6 / 2.1e-5
      fp32_mfma              1.9e-6 / 2.7e-6 / 1.9e-6 / 5.2e-6  |  4.8e-6 / 1.2e-6 / 5.2e-6 / 2.6e-5
    (the training-mode end of the stack is where tests/test_gpu_backward.py:127 measured its 2.1e-5)."""
    s = setup(dev, gammas)
    references_differ(s)
    out = run_mode(s, mode)
    check_stack(s, out, base_ref(s, mode), mode, "whole_stack %s %s %s" % (gammas, mode, FORMS[gemm_form]))
    for k in ("seeds_points", "votes_points", "proposals_output"):
        assert bool(torch.isfinite(out[k]).all())


@pytest.mark.parametrize("gammas,mode", CASES, ids=CASE_IDS)
def test_each_module_on_the_references_input(hiplib, dev, gemm_form, gammas, mode):
    """Every device module is fed the REFERENCE's input of that module (rounded to fp32), under frozen_bn(net.inference_bn()) -- or in
    training mode --, so an error is that module's own: sa1 (narrow first layer), sa2-sa4 and the proposal module (assembled first
    layer, piece layout), fp1, fp2, the voting chain.  Centres exact, features to MODULE_BAR."""
    from votenet_amd import mlp as M
    from votenet_amd import pointnet2 as P
    s = setup(dev, gammas)
    net, x = s["net"], s["x"]
    r = base_ref(s, mode)[0]
    T = lambda a: a.float().contiguous().to(dev)
    b = x.shape[0]
    # the forms these shapes select (what the untaped pass below runs)
    assert net.sa1.narrow(b * 512 * 64) and net.sa1.half_groups(b, 2048)
    for mod, n in ((net.sa2, 512), (net.sa3, 256), (net.sa4, 128), (net.proposal, 256)):
        assert mod.assembled(b, n) and mod.half_groups(b, n) and not mod.narrow(b * mod.npoint * 64)
    errs = {}
    with P.frozen_bn(net.inference_bn() if mode == "moving" else None):
        net.store.refresh_split()
        M.arena_begin(dev)
        try:
            for name, xin, pin, xo, po in (("sa1", None, None, "l1_xyz", "l1_p"), ("sa2", "l1_xyz", "l1_p", "l2_xyz", "l2_p"),
                                           ("sa3", "l2_xyz", "l2_p", "l3_xyz", "l3_p"), ("sa4", "l3_xyz", "l3_p", "l4_xyz", "l4_p")):
                xi, pi = (x, x) if xin is None else (T(r[xin]), T(r[pin]))
                cx, cp, cidx = getattr(net, name).forward(xi, pi)
                assert np.array_equal(cx.cpu().double().numpy(), r[xo].numpy()), name
                assert torch.equal(cidx.cpu(), s["geometry"][name]["idx"]), name  # the grouping the reference ran on
                errs[name] = R.relerr(cp, r[po])
            errs["fp1"] = R.relerr(net.fp1.forward(T(r["l3_xyz"]), T(r["l4_xyz"]), T(r["l3_p"]), T(r["l4_p"])), r["l3_p2"])
            errs["fp2"] = R.relerr(net.fp2.forward(T(r["l2_xyz"]), T(r["l3_xyz"]), T(r["l2_p"]), T(r["l3_p2"])), r["seeds_points"])
            vx, vp = net.vote(T(r["l2_xyz"]), T(r["seeds_points"]))
            errs["vote_xyz"], errs["vote_feat"] = R.relerr(vx, r["votes_xyz"]), R.relerr(vp, r["votes_points"])
            rvx, rvp, rsx = T(r["votes_xyz"]), T(r["votes_points"]), T(r["l2_xyz"])
            px, pout = net.propose(rvx, rvp, rsx)
        finally:
            M.arena_end()
    pg, new_xyz = proposal_geometry(net, rvx, rsx)
    assert torch.equal(px, new_xyz)
    ref, _ = propose(s, base_ref(s, mode), mode, pg)
    errs["proposal"] = R.relerr(pout.view(b, 256, 79), ref["proposals_output"])
    print("MEASURED module_on_reference_input %s %s %s: %s" % (gammas, mode, FORMS[gemm_form], "  ".join("%s=%.2e" % kv for kv in errs.items())))
    # measured, worst module over the three cases: fp16x2_forward_images 1.0e-6 (fp2), bf16x3_images 1.2e-6 (fp2), fp32_mfma 1.5e-6 (proposal)
    assert max(errs.values()) < MODULE_BAR, errs


@pytest.mark.parametrize("switch", ["HALF_GROUPS", "ASSEMBLE_FIRST", "NARROW_FIRST", "POOL_IN_EPILOGUE"])
def test_whole_stack_on_every_layout(hiplib, dev, switch):
    """predict(x) with one layout switch off at a time (the full grouped rows; the stored per-point first layer; sa1's first layer
    stored; the pool as its own pass over z), signed gammas, the default GEMM form, a fresh net per setting: the same reference."""
    from votenet_amd import pointnet2 as P
    assert getattr(P, switch) is True
    setattr(P, switch, False)
    try:
        s = setup(dev, "signed")
        b = s["x"].shape[0]
        if switch in ("HALF_GROUPS", "POOL_IN_EPILOGUE"):
            assert not any(m.half_groups(b, n) for m, n in ((s["net"].sa1, 2048), (s["net"].sa2, 512), (s["net"].proposal, 256)))
        if switch == "ASSEMBLE_FIRST":
            assert not s["net"].sa2.assembled(b, 512) and not s["net"].proposal.assembled(b, 256)
        if switch == "NARROW_FIRST":
            assert not s["net"].sa1.narrow(b * 512 * 64)
        out = run_mode(s, "moving")
        check_stack(s, out, base_ref(s, "moving"), "moving", "whole_stack signed moving %s=False" % switch)
    finally:
        setattr(P, switch, True)


def test_taped_and_untaped_inference_are_the_same_pass(hiplib, dev):
    """forward(x, tape) and forward(x) under the same frozen table: keep_z only drops a store, so the outputs are bit-equal; the taped
    run's records show which forms ran (narrow / assembled first layers, the piece layout), and both hold the float64 bar."""
    s = setup(dev, "signed")
    tape = []
    taped = run_mode(s, "moving", tape)
    untaped = run_mode(s, "moving", None)
    sa = [tape[i] for i in (0, 1, 2, 3, 7)]
    assert [t["recs"][0]["kind"] for t in sa] == ["narrow", "assembled", "assembled", "assembled", "assembled"]
    assert all(t["recs"][0]["half"] is not None for t in sa)
    for t in sa:  # inference mode: the table's entries, no batch statistics recorded; the pooled layer's z is not stored in Gram form
        assert all("mean" not in r for r in t["recs"] + t["recs2"]) and t["recs"][-1]["pool"] is not None
    base = base_ref(s, "moving")
    check_stack(s, taped, base, "moving", "taped signed moving")
    check_stack(s, untaped, base, "moving", "untaped signed moving")
    same = {k: bool(torch.equal(taped[k], untaped[k])) for k in CHAINED + ("proposals_xyz", "proposals_output")}
    print("MEASURED taped == untaped: %s" % same)
    assert all(same.values()), same  # measured: every output bit-equal


def test_batch_of_one_and_of_three_scene_by_scene(hiplib, dev):
    """b = 1 and b = 3 through predict(x): every scene within the bars of the float64 reference of THAT SCENE ALONE -- the batch-mate
    independence of inference mode, against a reference (test_gpu_model's states it device against device)."""
    s = setup(dev, "signed")
    net = s["net"]
    x3 = torch.from_numpy(scenes(3)).to(dev)
    assert torch.equal(x3[:2], s["x"])
    g3 = fresh_geometry(net, x3)
    for k in ("sa1", "sa4", "fp2"):  # (the first two scenes: the indices the taped pass of the set-up ran on)
        assert torch.equal(g3[k]["idx"][:2], s["geometry"][k]["idx"]), k
    out3 = net.predict(x3)
    out1 = net.predict(x3[:1].contiguous())
    torch.cuda.synchronize()
    for sc in range(3):
        base = base_ref(s, "moving", scene=sc, geometry=scene_of(g3, sc), x=x3[sc:sc + 1])
        check_stack(s, out3, base, "moving", "b=3 scene %d alone" % sc, slice(sc, sc + 1))
    check_stack(s, out1, base_ref(s, "moving", scene=0), "moving", "b=1 scene 0")


@pytest.mark.parametrize("shape", ["balls", "group_all"])
@pytest.mark.parametrize("pooling", ["avg", "weighted_avg", "max_and_avg", "max"])
def test_stand_alone_sa_module_under_a_hand_built_table(hiplib, dev, monkeypatch, pooling, shape):
    """SAModule by itself under frozen_bn(table) with hand-built mlp.FrozenBN entries: every pooling mode on small balls with padding
    and an empty ball, and group_all at n = 1000 (the shapes of tests/test_gpu_sa_pooling.py), signed gammas.  The reference is that
    file's ref_sa with the moving statistics in place of the batch's.  (_forward_plain_pool's pend.finalize() on a FrozenBN.)"""
    import test_gpu_sa_pooling as SP
    from votenet_amd import mlp as M
    from votenet_amd import pointnet2 as P
    if shape == "balls":
        store, mod = SP.build(dev, 48, 0.15, 16, 6, [32, 64], pooling=pooling)
        xyz, pts = SP.small_cloud(dev, 2, 600, 6)
        fps_idx, new_xyz, _, _ = P.sample_and_group(48, 0.15, 16, xyz)
        shift = torch.zeros_like(new_xyz)
        shift[1, 5] = 50.0
        moved = new_xyz + shift
        idx, cnt = P.tf_grouping.query_ball_point(0.15, 16, xyz, moved)
        assert int(cnt[1, 5]) == 0 and bool((cnt < 16).any())
        geom = P.SAGeometry(fps_idx, moved, M.attach_inverse(idx, 600), cnt)
        centre_shift = (moved.double() - new_xyz.double()).cpu()
    else:
        store, mod = SP.build(dev, 99, 0.1, 7, 6, [32, 64], pooling=pooling, group_all=True)
        g = torch.Generator().manual_seed(6)
        xyz = (torch.rand(2, 1000, 3, generator=g) * 2 - 1).to(dev)
        xyz[0, 7] = 0.0
        pts = torch.randn(2, 1000, 6, generator=g).to(dev)
        geom, centre_shift = None, None
    g = torch.Generator().manual_seed(9)
    table, stats = {}, {}
    for L in mod.mlp:
        gamma = 0.2 + 0.3 * torch.randn(L.cout, generator=g, dtype=torch.float64)
        gamma[::7] = 0.0
        assert bool((gamma < 0).any())
        store[L.name + "/gamma"].copy_(gamma.float().to(dev))
        gamma = gamma.float().double()
        beta = store[L.name + "/beta"].cpu().double()
        mm = (0.3 * torch.randn(L.cout, generator=g, dtype=torch.float64)).float().double()
        mv = (0.5 + 1.5 * torch.rand(L.cout, generator=g, dtype=torch.float64)).float().double()
        scale = gamma / torch.sqrt(mv + M.BN_EPS)
        table[L.name] = M.FrozenBN(torch.stack([scale, beta - mm * scale]).float().contiguous().to(dev))
        stats[L.name] = (mm, mv)
    store.params_changed()
    tape = []
    with P.frozen_bn(table):
        new_xyz_d, out, _ = mod.forward(xyz, pts, tape=tape, geom=geom)
    torch.cuda.synchronize()
    rec = tape[0]
    assert all("mean" not in r for r in rec["recs"])  # the table's entries were used, not the launches' sums

    def moving_chain(x, layers, params, recs):
        return R.chain_ref(x, [R.Layer(L.name, L.bn, L.relu) for L in layers], params, stats, "moving")
    monkeypatch.setattr(SP, "ref_chain", moving_chain)
    cpu = lambda v: v.cpu() if torch.is_tensor(v) else v
    rec_cpu = {k: cpu(v) for k, v in rec.items()}
    params = {k: v.detach().cpu().double() for k, v in store.views.items()}
    rnew, y = SP.ref_sa(mod, params, xyz.cpu().double(), pts.cpu().double(), rec_cpu, centre_shift)
    assert torch.equal(new_xyz_d.cpu().double(), rnew)
    e = R.relerr(out, y)
    print("MEASURED stand_alone_sa %s %s: %.2e" % (shape, pooling, e))
    assert e < MODULE_BAR, e  # measured: <= 1.7e-7 over the eight cases


def test_moving_averages_of_all_23_layers_vs_float64(hiplib, dev):
    """One training-mode forward pass from the initial 0 / 1 state and update_moving_averages(tape): for ALL 23 BatchNorm layers -- the
    narrow and assembled first layers and the Gram-form pooled layers included, whose z no kernel stores -- moving_mean = 0.1 mean64 and
    moving_var = 0.9 + 0.1 var64_unbiased, mean64 / var64 from the float64 reference's z of that layer (batch mode, the tape's own
    indices).  Judged as tests/bn_stats_ref.py judges statistics: e = max |a_dev - a_ref| / max(1, max |a_ref|) on the layer's
    normalised output a -- here the output inference forms from the two sets of moving statistics -- under that file's BAR."""
    import bn_stats_ref as B
    net = make_net(dev, "perturbed")
    x = torch.from_numpy(scenes()).to(dev)
    ema = net._ema_state()
    assert all(bool((t[2] == 0).all()) and bool((t[3] == 1).all()) for t in ema.values())
    tape = []
    net.forward(x, tape)
    net.update_moving_averages(tape)
    torch.cuda.synchronize()
    kinds = {r["layer"].name: r["kind"] for r in net._bn_records(tape)}
    unstored = [n for n, r in ((r["layer"].name, r) for r in net._bn_records(tape)) if r["z"] is None]
    assert kinds["sa1/conv0"] == "narrow" and kinds["sa2/conv0"] == "assembled" and kinds["proposal/conv0"] == "assembled"
    assert set(unstored) >= {"sa%d/conv%d" % (i, j) for i in (1, 2, 3, 4) for j in (0, 2)} | {"proposal/conv0", "proposal/conv2"}
    s = dict(gammas="perturbed", params=params_of(net), stats=None, geometry=tape_geometry(tape), x=x)  # (the batch-mode reference of the set)
    base = base_ref(s, "batch")
    _, bn = propose(s, base, "batch", dict(fps_idx=tape[7]["fps_idx"].cpu(), idx=tape[7]["idx"].cpu()))
    assert sorted(bn) == sorted(ema) and len(bn) == 23
    errs = {}
    for name, rec in bn.items():
        want = (0.1 * rec["mean"], 0.9 + 0.1 * rec["var_unbiased"])
        errs[name] = R.moving_error(rec, s["params"][name + "/gamma"], s["params"][name + "/beta"], (ema[name][2], ema[name][3]), want)
        assert rec["rows"] == next(r["rows"] for r in net._bn_records(tape) if r["layer"].name == name)
    worst = max(errs, key=errs.get)
    print("MEASURED moving_averages: worst %s=%.2e  %s" % (worst, errs[worst], "  ".join("%s=%.1e" % kv for kv in errs.items())))
    assert errs[worst] < B.BAR, (worst, errs[worst])  # measured: 2.4e-8 (sa1/conv0) .. 1.4e-7 (proposal/conv0)
    for name in bn:  # no layer was left in the initial state
        assert bool((ema[name][2] != 0).any()) and bool((ema[name][3] != 1).any()), name
