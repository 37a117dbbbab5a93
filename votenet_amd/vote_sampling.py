"""The proposal module's clusters sampled by farthest-point sampling on the VOTES, as the VoteNet paper does, on the device
(libvotenet_votesamp.so, include/votenet_vote_sampling.h).

The reference calls pointnet_sa_module(votes_xyz, ..., sample_xyz=seeds_xyz) (model.py:89-93, utils.py:42-43): its 256 cluster centres
are the votes of the 256 seeds that farthest-point sampling picks among the SEEDS.  The paper samples among the votes (`vote_fps`, its
default): votes are trained to pile up at object centres, so sampling them covers objects, sampling seeds covers surfaces.

cluster_votes is one launch, one workgroup per scene: what tf_sampling.farthest_point_sample(npoint, votes), tf_sampling.gather_point
and tf_grouping.query_ball_point leave on the same votes, bit for bit (five dependent launches in the middle of the step's static
stretch, where the votes first exist).  VoteNetHotPath.enable_proposal_sampling("vote_fps") hands its result to the proposal module in
every pass.  The rule is stated once, in the header; tests/vote_sampling_ref.py restates it in numpy.

Not taken over from the paper (out of scope here): its `random` sampling mode."""
import torch

from . import _lib as L

MODES = ("seed_fps", "vote_fps")  # "seed_fps": the reference's rule, the default, no launch of this library
MAX_N, MAX_M, MAX_NSAMPLE = 2048, 1024, 64  # the kernel's limits (the header's)


def supported(n, m, nsample):
    """True when cluster_votes takes n votes, m clusters and nsample votes per cluster."""
    return bool(1 <= n <= MAX_N and 1 <= m <= MAX_M and 1 <= nsample <= MAX_NSAMPLE)


def cluster_votes(votes_xyz, npoint, radius, nsample):
    """votes_xyz (B,n,3) f32 -> fps_idx (B,npoint) int32, new_xyz (B,npoint,3) f32, idx (B,npoint,nsample) int32, pts_cnt (B,npoint)
    int32: the votes' farthest-point sample, the raw votes there, and their ball query.  One launch, nothing is read back."""
    v = L.dev_f32(votes_xyz.detach(), "cluster_votes expects (batch_size,num_votes,3) votes_xyz shape", 3, 3)
    b, n, _ = v.shape
    m, k = int(npoint), int(nsample)
    dev = v.device
    fps_idx = torch.empty((b, max(m, 0)), dtype=torch.int32, device=dev)
    new_xyz = torch.empty((b, max(m, 0), 3), dtype=torch.float32, device=dev)
    idx = torch.empty((b, max(m, 0), max(k, 0)), dtype=torch.int32, device=dev)
    pts_cnt = torch.empty((b, max(m, 0)), dtype=torch.int32, device=dev)
    with L.device_guard(dev):
        L.check(L.side_lib("votesamp").votenet_cluster_votes(b, n, m, float(radius), k, L.ptr(v), L.ptr(fps_idx), L.ptr(new_xyz),
                                                             L.ptr(idx), L.ptr(pts_cnt), L.stream_ptr()), side="votesamp")
    return fps_idx, new_xyz, idx, pts_cnt
