"""The layer stack of votenet_amd/model.py (sa1-sa4, fp1, fp2, the voting chain with its residual, the proposal module with mlp2)
restated in float64 on the CPU (torch), with BatchNorm either in inference mode -- the moving averages, what VoteNetHotPath.predict
runs -- or in training mode -- biased batch statistics, as tests/test_gpu_backward.py:ref_chain states them.  No device code, the
package is not imported: parameters, moving statistics and indices arrive as plain arrays under the names the package gives them.

forward_ref()    the whole stack; every module's output and, per BatchNorm layer, the float64 statistics of its z
chain_ref()      one MLP chain: z = x W + b, BatchNorm (moving | batch), ReLU, layer by layer
sa_ref() / fp_ref() / vote_ref()   the modules
moving_error()   the bar shape of tests/bn_stats_ref.py:metric on a layer's normalised output, for two sets of MOVING statistics

The forward pass is continuous in its inputs (relu, max), so no active set of the device is needed: a plain relu / max is right."""
import collections

import numpy as np
import torch

BN_EPS = 1e-5        # TensorFlow / Tensorpack BatchNorm epsilon (votenet_amd.mlp.BN_EPS)
BN_MOMENTUM = 0.9    # Tensorpack BatchNorm momentum (VoteNetHotPath.BN_MOMENTUM)

Layer = collections.namedtuple("Layer", "name bn relu")


def mlp_spec(scope, n, prefix="conv", last_plain=False):
    """The layers pointnet2.make_mlp declares: <scope>/<prefix><i>, BatchNorm + ReLU on all but a plain last one."""
    return [Layer("%s/%s%d" % (scope, prefix, i), not (last_plain and i == n - 1), not (last_plain and i == n - 1)) for i in range(n)]


# model.py (VoteNetHotPath.__init__): module -> its chain(s)
STACK = dict(sa1=mlp_spec("sa1", 3), sa2=mlp_spec("sa2", 3), sa3=mlp_spec("sa3", 3), sa4=mlp_spec("sa4", 3),
             fp1=mlp_spec("fp1", 2, "conv_"), fp2=mlp_spec("fp2", 2, "conv_"), voting=mlp_spec("voting", 3, "fc", last_plain=True),
             proposal=mlp_spec("proposal", 3), proposal_post=mlp_spec("proposal", 3, "conv_post_", last_plain=True))
MODULES = ("sa1", "sa2", "sa3", "sa4", "fp1", "fp2", "voting", "proposal", "proposal_post")  # the order the pass runs them in


def bn_layer_names():
    """The 23 BatchNorm layers in the order of a forward pass."""
    return [L.name for m in MODULES for L in STACK[m] if L.bn]


def f64(a):
    if torch.is_tensor(a):
        return a.detach().to("cpu", torch.float64)
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64)


def i64(a):
    if torch.is_tensor(a):
        return a.detach().to("cpu", torch.int64)
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.int64)


def chain_ref(x, layers, params, stats, mode, bn=None):
    """x (rows, cin) float64 through `layers` (Layer records).  params: name + "/W" | "/b" | "/gamma" | "/beta" -> array.
    mode "moving": y = gamma (z - moving_mean) / sqrt(moving_var + eps) + beta with stats[name] = (moving_mean, moving_var);
    mode "batch": the mean and the BIASED variance of z over its rows.
    bn (a dict, optional) receives per BatchNorm layer the float64 batch statistics of ITS z in either mode: mean, var (biased),
    var_unbiased, rows, and the per-channel extremes zmin / zmax (an affine function of z takes its extremes there)."""
    if mode not in ("moving", "batch"):
        raise ValueError("mode must be 'moving' or 'batch', got %r" % (mode,))
    for L in layers:
        z = x @ f64(params[L.name + "/W"]) + f64(params[L.name + "/b"])
        if L.bn:
            rows = z.shape[0]
            mean = z.mean(0)
            d = z - mean
            var = (d * d).mean(0)
            if bn is not None:
                bn[L.name] = dict(mean=mean, var=var, var_unbiased=var * (rows / max(rows - 1.0, 1.0)), rows=rows,
                                  zmin=z.amin(0), zmax=z.amax(0))
            if mode == "moving":
                mean, var = f64(stats[L.name][0]), f64(stats[L.name][1])
            z = f64(params[L.name + "/gamma"]) * (z - mean) / torch.sqrt(var + BN_EPS) + f64(params[L.name + "/beta"])
        if L.relu:
            z = torch.relu(z)
        x = z
    return x


def group_rows(xyz, points, fps_idx, idx):
    """sample_and_group's concat on given indices: -> new_xyz (b, m, 3), rows (b, m, k, 3 + c) = [xyz[idx] - new_xyz | points[idx]]."""
    b = xyz.shape[0]
    bi = torch.arange(b)
    new_xyz = xyz[bi[:, None], fps_idx]
    g = xyz[bi[:, None, None], idx] - new_xyz[:, :, None, :]
    if points is not None:
        g = torch.cat([g, points[bi[:, None, None], idx]], -1)
    return new_xyz, g


def sa_ref(layers, params, stats, mode, xyz, points, fps_idx, idx, bn=None, post=None):
    """pointnet_sa_module with max pooling on given indices: grouped concat -> MLP -> BN -> ReLU -> max over k [-> mlp2]."""
    b, m, k = idx.shape
    new_xyz, g = group_rows(xyz, points, fps_idx, idx)
    y = chain_ref(g.reshape(b * m * k, -1), layers, params, stats, mode, bn).view(b * m, k, -1).amax(1)
    if post:
        y = chain_ref(y, post, params, stats, mode, bn)
    return new_xyz, y.view(b, m, -1)


def fp_ref(layers, params, stats, mode, points1, points2, idx, weight, bn=None):
    """pointnet_fp_module on given taps: three taps x weights, concat [interpolated | points1], MLP."""
    b, n1 = idx.shape[:2]
    interp = (points2[torch.arange(b)[:, None, None], idx] * weight[..., None]).sum(2)
    x = torch.cat([interp, points1], 2)
    return chain_ref(x.view(b * n1, -1), layers, params, stats, mode, bn).view(b, n1, -1)


def vote_ref(layers, params, stats, mode, seeds_xyz, seeds_points, bn=None):
    """votes = [seeds_xyz | seeds_points] + FC chain of it -> votes_xyz (b, n, 3), votes_points (b, n, c)."""
    b, n = seeds_xyz.shape[:2]
    x = torch.cat([seeds_xyz, seeds_points], 2).view(b * n, -1)
    v = (x + chain_ref(x, layers, params, stats, mode, bn)).view(b, n, -1)
    return v[..., :3], v[..., 3:]


def forward_ref(params, stats, geometry, x, mode, stack=None):
    """The stack of model.py on x (b, n, 3) in float64.
    params: name -> array (the ParamStore's views).  stats: layer name -> (moving_mean, moving_var); read in mode "moving" only.
    geometry: "sa1".."sa4" -> dict(fps_idx (b, m), idx (b, m, k)); "fp1", "fp2" -> dict(idx (b, n1, 3), weight (b, n1, 3), the fp32
    weights as they are); "proposal" -> dict(fps_idx, idx), or a callable(votes_xyz float64 tensor) returning that dict (the
    proposal module's neighbour lists depend on the votes of the run they serve), or None: the pass stops behind the votes (propose_ref
    completes it).
    -> (out, bn): out holds every module's output as float64 tensors -- l1_xyz, l1_p .. l4_xyz, l4_p, l3_p2 (fp1), seeds_xyz,
    seeds_points (fp2), votes_xyz, votes_points, proposals_xyz, proposals_output; bn: layer name -> the statistics chain_ref leaves."""
    S = stack or STACK
    bn = {}
    x = f64(x)
    o = {}
    xyz, pts = x, x  # sa1's input features are the coordinates themselves
    for i, name in enumerate(("sa1", "sa2", "sa3", "sa4"), 1):
        g = geometry[name]
        xyz, pts = sa_ref(S[name], params, stats, mode, xyz, pts, i64(g["fps_idx"]), i64(g["idx"]), bn)
        o["l%d_xyz" % i], o["l%d_p" % i] = xyz, pts
    g = geometry["fp1"]
    o["l3_p2"] = fp_ref(S["fp1"], params, stats, mode, o["l3_p"], o["l4_p"], i64(g["idx"]), f64(g["weight"]), bn)
    g = geometry["fp2"]
    o["seeds_points"] = fp_ref(S["fp2"], params, stats, mode, o["l2_p"], o["l3_p2"], i64(g["idx"]), f64(g["weight"]), bn)
    o["seeds_xyz"] = o["l2_xyz"]
    o["votes_xyz"], o["votes_points"] = vote_ref(S["voting"], params, stats, mode, o["seeds_xyz"], o["seeds_points"], bn)
    if geometry.get("proposal") is not None:
        propose_ref(params, stats, geometry["proposal"], o, mode, bn, stack)
    return o, bn


def propose_ref(params, stats, g, o, mode, bn=None, stack=None):
    """The proposal module on o["votes_xyz"] / o["votes_points"] (what forward_ref left; with geometry["proposal"] = None it stops
    behind the votes, so that one run of the levels serves several groupings of its votes).  g: dict(fps_idx, idx) or a callable of the
    votes' coordinates.  Adds proposals_xyz / proposals_output to o (and the module's layers to bn) and returns the two."""
    S = stack or STACK
    if callable(g):
        g = g(o["votes_xyz"])
    o["proposals_xyz"], o["proposals_output"] = sa_ref(S["proposal"], params, stats, mode, o["votes_xyz"], o["votes_points"],
                                                       i64(g["fps_idx"]), i64(g["idx"]), bn, post=S["proposal_post"])
    return o["proposals_xyz"], o["proposals_output"]


def relerr(got, ref):
    """The project's bar shape: max |got - ref| / max(1, max |ref|)."""
    got, ref = f64(got), f64(ref)
    return float((got - ref).abs().max() / max(1.0, float(ref.abs().max())))


def moving_error(rec, gamma, beta, got, want):
    """e of tests/bn_stats_ref.py:metric -- max |a_dev - a_ref| / max(1, max |a_ref|) on the layer's normalised output
    a = gamma (z - mean) / sqrt(var + eps) + beta -- for the two sets of MOVING statistics got = (mean, var) (the device's) and want
    (the reference's), over the z of the reference (rec: what chain_ref left of it).  a is affine in z per channel, so both maxima are
    taken at the channel's zmin / zmax."""
    gamma, beta = f64(gamma), f64(beta)

    def affine(mean, var):
        s = gamma / torch.sqrt(f64(var) + BN_EPS)
        return s, beta - f64(mean) * s
    (sd, hd), (sr, hr) = affine(*got), affine(*want)
    ends = torch.stack([rec["zmin"], rec["zmax"]])
    den = max(1.0, float((ends * sr + hr).abs().max()))
    return float((ends * (sd - sr) + (hd - hr)).abs().max()) / den
