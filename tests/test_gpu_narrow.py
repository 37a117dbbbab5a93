"""GPU: the narrow-first-layer kernels (csrc/narrow.hip, SRC 3 / EPI 4 of mlp_fast.hip, MODE 2 of mlp_wgrad_fast.hip) against
float64 torch over the materialised grouped tensor [xyz[idx]-new_xyz | feat[idx]] (utils.py:50-57,125-127): the first layer's
output is never stored on the device, so every quantity is checked against the layer computed the ordinary way."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def relerr(a, b):
    return float((a.double() - b.double()).abs().max() / max(1e-12, float(b.double().abs().max())))


def setup(dev, b, n, m, k, c, c0, c1, seed):
    from votenet_amd import tf_grouping, tf_sampling
    g = torch.Generator().manual_seed(seed)
    xyz = (torch.rand(b, n, 3, generator=g) * 2.0).to(dev)
    feat = torch.randn(b, n, c, generator=g).to(dev) if c else None
    fi = tf_sampling.farthest_point_sample(m, xyz)
    new_xyz = tf_sampling.gather_point(xyz, fi)
    idx, _ = tf_grouping.query_ball_point(0.6, k, xyz, new_xyz)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    w0, b0 = rnd(3 + c, c0) * 0.5, rnd(c0) * 0.1
    w1 = rnd(c0, c1) * 0.2
    bi = torch.arange(b, device=dev)[:, None, None]
    rows_in = xyz[bi, idx.long()] - new_xyz[:, :, None, :]
    if c:
        rows_in = torch.cat([rows_in, feat[bi, idx.long()]], -1)
    return xyz, new_xyz, feat, idx, w0, b0, w1, rows_in.reshape(b * m * k, 3 + c), rnd


@pytest.mark.parametrize("b,n,m,k,c,c0,c1", [(2, 500, 64, 64, 3, 64, 64), (1, 300, 32, 64, 1, 128, 128), (2, 256, 16, 64, 0, 64, 128),
                                             (1, 400, 8, 16, 5, 64, 64)])
def test_narrow_first_layer_matches_the_materialised_layer(hiplib, dev, gemm_form, b, n, m, k, c, c0, c1):
    narrow_first_layer(dev, gemm_form, b, n, m, k, c, c0, c1)


def narrow_first_layer(dev, gemm_form, b, n, m, k, c, c0, c1, run=None):
    """The body of the test above.  run(tag, fn) -> fn(): how the two fused GEMMs are launched (tests/test_gpu_tile_walk.py launches them
    under its workgroup caps and hands back the walked launch's results); -> the rows of the GEMMs."""
    from votenet_amd import mlp as M
    run = run or (lambda tag, fn: fn())
    xyz, new_xyz, feat, idx, w0, b0, w1, rows_in, rnd = setup(dev, b, n, m, k, c, c0, c1, 7 * n + c)
    wT = w1.t().contiguous()
    # images for the second layer's forward GEMM (fp16 x 2 when gemm_form == 2, as the model registers its forward matrices) and its
    # input-gradient GEMM (the transposed copy: always bf16 x 3); gemm_form == 0 ignores them
    img_f = M.SplitImages([w1], pieces=2 if gemm_form == 2 else 3)
    img_f.refresh()
    img = M.SplitImages([wT])
    img.refresh()
    rows, k0 = rows_in.shape
    assert M.narrow_supported(rows, k0, c0, c1)
    # u8 and its moments
    u8, mom = M.narrow_rows(xyz, new_xyz, feat, idx)
    assert torch.equal(u8[:, :k0], rows_in) and float(u8[:, k0:].abs().max()) == 0.0 if k0 < 8 else torch.equal(u8, rows_in)
    ud = u8.double()
    assert relerr(mom[:8], ud.sum(0)) < 1e-12 and relerr(mom[8:].view(8, 8), ud.t() @ ud) < 1e-12
    # BatchNorm statistics of the never-stored z0
    z0 = rows_in.double() @ w0.double() + b0.double()
    st = M.narrow_stats(rows, mom, w0, b0)
    assert relerr(st[:c0], z0.sum(0)) < 1e-10 and relerr(st[c0:], (z0 * z0).sum(0)) < 1e-10
    gamma0, beta0 = rnd(c0) * 0.2 + 1.0, rnd(c0) * 0.1
    bn0 = M.PendingBN(st, gamma0, beta0, rows)
    # second layer forward: z1 and its statistics
    z1, st1 = run("narrow", lambda: M.narrow_linear(u8, w0, b0, w1, None, bn0))
    mu, var = z0.mean(0), z0.var(0, unbiased=False)
    assert relerr(bn0.mean, mu) < 1e-6 and relerr(bn0.var, var) < 1e-5
    a0 = torch.relu(gamma0.double() * (z0 - mu) / torch.sqrt(var + M.BN_EPS) + beta0.double())
    z1_ref = a0 @ w1.double()
    assert relerr(z1, z1_ref) < 2e-5
    assert relerr(st1[:c1], z1_ref.sum(0)) < 2e-5 and relerr(st1[c1:], (z1_ref * z1_ref).sum(0)) < 2e-5
    # the finalized form of the same BatchNorm (second consumer: scale / shift vectors)
    z1b, _ = M.narrow_linear(u8, w0, b0, w1, None, bn0)
    assert torch.equal(z1b, z1)
    # backward of the second layer: random upstream gradient and coefficients
    da1, coef1 = rnd(rows, c1), rnd(5 * c1)
    g1 = da1.double() * (z1.double() * coef1[3 * c1:4 * c1].double() + coef1[4 * c1:].double() > 0)
    dz1 = coef1[:c1].double() * g1 + coef1[c1:2 * c1].double() + coef1[2 * c1:3 * c1].double() * z1.double()
    dw1 = torch.zeros(c0, c1, device=dev)
    M.narrow_wgrad_bn(u8, w0, b0, bn0.scale, bn0.shift, True, z1, coef1, True, da1, dw1)
    a0f = torch.relu((u8[:, :k0].double() @ w0.double() + b0.double()) * bn0.scale.double() + bn0.shift.double())
    assert relerr(dw1, a0f.t() @ dz1) < 2e-5
    sums, ug = run("narrow_dgrad", lambda: M.narrow_dgrad_bn_reduce(z1, coef1, True, wT, da1, u8, w0, b0, (bn0.scale, bn0.shift, bn0.mean, bn0.var, True)))
    da0 = dz1 @ w1.double().t()
    act = (z0 * bn0.scale.double() + bn0.shift.double()) > 0
    # entries whose pre-activation is within fp32 rounding of zero may take either side: they carry |da0| each, far below the bound
    g0 = da0 * act
    zh = (z0 - bn0.mean.double()) / torch.sqrt(bn0.var.double() + M.BN_EPS)
    scale1, scale2 = da0.abs().sum(0), (da0 * zh).abs().sum(0)
    assert float(((sums[:c0] - g0.sum(0)).abs() / scale1).max()) < 2e-5
    assert float(((sums[c0:] - (g0 * zh).sum(0)).abs() / scale2).max()) < 2e-5
    ug_ref = ud.t() @ g0
    assert float(((ug - ug_ref).abs() / (ud.abs().t() @ da0.abs() + 1e-30)).max()) < 2e-5
    # first layer's weight gradient from the sums alone
    coef0 = rnd(5 * c0)
    dz0 = coef0[:c0].double() * g0 + coef0[c0:2 * c0].double() + coef0[2 * c0:3 * c0].double() * z0
    dw0 = torch.zeros(k0, c0, device=dev)
    M.narrow_wgrad_first(mom, ug, coef0, w0, b0, dw0)
    assert relerr(dw0, ud[:, :k0].t() @ dz0) < 2e-5
    img.close()
    img_f.close()
    return rows


def test_narrow_kernels_reject_unserved_shapes(hiplib, dev):
    from votenet_amd import _lib, mlp as M
    assert not M.narrow_supported(1000, 6, 64, 64) and not M.narrow_supported(1024, 9, 64, 64) and not M.narrow_supported(1024, 6, 96, 64)
    u8 = torch.zeros(1024, 8, device=dev)
    w0, b0 = torch.zeros(6, 256, device=dev), torch.zeros(256, device=dev)
    bn = M.PendingBN(torch.ones(512, dtype=torch.float64, device=dev), torch.ones(256, device=dev), torch.zeros(256, device=dev), 1024)
    with pytest.raises(_lib.InvalidArgumentError):
        M.narrow_linear(u8, w0, b0, torch.zeros(256, 64, device=dev), None, bn)  # c0 > 128


def test_model_with_and_without_the_narrow_first_layer(hiplib, dev):
    """The whole hot path (forward, loss graph, backward) with sa1's first layer in the narrow form against the same network with
    that layer in the per-point form (votenet_group_linear or csrc/assemble.hip, + the scatter of its backward): same outputs, same gradient bucket to fp32
    rounding -- and the narrow form really is the one that runs by default."""
    from votenet_amd import loss as VL
    from votenet_amd import model as VM
    from votenet_amd import pointnet2 as P
    from votenet_amd import synth
    b, n = 2, 4096
    x = torch.from_numpy(synth.room_batch(b, n, 5)).to(dev)
    gt = VL.gt_to_device(synth.room_gt(b, n, 5), dev)
    net = VM.VoteNetHotPath(dev, seed=4, npoints=(512, 256, 128, 64))

    fixed = {}

    def once():
        net.store.grad.zero_()
        net.store.refresh_transposes()
        tape = []
        out = net.forward(x, tape)
        losses, cot = VL.votenet_loss(out, gt)
        # both passes back-propagate the FIRST pass's cotangents: the loss graph takes discrete decisions (label assignment,
        # objectness thresholds) that an fp32-rounding difference in the outputs may flip, which says nothing about the layer
        cot = fixed.setdefault("cot", cot)
        net.backward(tape, cot)
        torch.cuda.synchronize()
        return tape, out["proposals_output"].clone(), losses.clone(), net.store.grad.clone()
    assert P.NARROW_FIRST
    tape, o1, l1, g1 = once()
    assert tape[0]["recs"][0]["kind"] == "narrow" and tape[0]["recs"][0]["z"] is None
    P.NARROW_FIRST = False
    try:
        tape, o0, l0, g0 = once()
        assert tape[0]["recs"][0]["kind"] in ("gather", "assembled")  # the per-point form: stored, or assembled in its consumers
    finally:
        P.NARROW_FIRST = True
    assert relerr(o1, o0) < 5e-5 and relerr(l1, l0) < 5e-5  # two fp32 evaluations, 26 layers deep (measured 2.0e-5)
    # Gradients: two fp32 evaluations of the forward pass differ in the last bits, which moves a few ReLU / arg-max decisions in
    # EVERY layer downstream (measured: the tensors of sa2..fp2, which this layer does not touch, differ by 1e-3..1e-2 of their
    # largest entry, against 1e-6 between two runs of one form).  The exact check of the narrow backward is
    # test_full_backward_vs_autograd (float64 autograd over the device's own active set); here: same gradient in the L2 sense.
    names = [nm for nm, _, _ in net.store._specs if nm.startswith("sa1/")]
    assert len(names) >= 10
    for name in names:
        a = net.store.g(name)
        o = a.storage_offset()
        v1, v0 = g1[o:o + a.numel()].double(), g0[o:o + a.numel()].double()
        if float(v0.abs().max()) > 0:  # bias gradients of BatchNorm'ed layers are identically zero
            assert float((v1 - v0).norm() / v0.norm()) < 1e-2, name
    assert float((g1.double() - g0.double()).norm() / g0.double().norm()) < 1e-2
