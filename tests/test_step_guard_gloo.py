"""CPU, world_size 2 over gloo: the step guard on the data-parallel path.  The REAL train_step host path on two ranks with the kernels
stubbed (tests/test_dp_gloo.py's stand-ins); the guarded optimizer entry is replaced by the restatement of tests/step_guard_cases.py
and step_guard.apply_rules.  One rank poisons its OWN gradient: the verdict is formed on the all-reduced bucket, so both replicas skip
the step, stay identical, and go on training."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _restated_clip_adam_guarded(seg, sumsq, p, g, m, v, lr, step, guard_state, ema=None, ema_snapshot=None, grad_scale=1.0, **kw):
    import step_guard_cases as C
    from test_dp_gloo import _torch_clip_adam
    from votenet_amd import step_guard as SG
    segs = list(zip(seg.tolist()[0::2], seg.tolist()[1::2]))
    bad = C.verdict(g.numpy(), segs)
    ema_bad = ema is not None and not bool(torch.isfinite(ema).all())
    new, restore = SG.apply_rules(guard_state.tolist()[:6], bad, ema_bad, step, have_ema=ema is not None)
    guard_state[:6] = torch.tensor(new, dtype=torch.int32)
    if ema is not None:
        (ema if restore else ema_snapshot).copy_(ema_snapshot if restore else ema)
    if not bad:
        _torch_clip_adam(seg, sumsq, p, g, m, v, lr, step, grad_scale=grad_scale)


def _guard_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from test_dp_gloo import _stub_net
    from votenet_amd import dp
    from votenet_amd import mlp as M
    events, step_no = [], [0]
    B = 2
    net = _stub_net(rank, rank, events, step_no, B)
    M.clip_adam_guarded = _restated_clip_adam_guarded
    dp.broadcast_params(net.store)
    net._gsync = dp.GradSync(net.store, net.store.offset_of("sa3/"))
    net.init_optimizer(lr=1e-3)
    guard = net.enable_step_guard()
    real_sa1 = net.sa1.backward

    def poisoned_sa1(rec, g_out, **kw):  # rank 1 only, step 2 only: ONE NaN in its own sa1 gradient, before the head all-reduce
        out = real_sa1(rec, g_out, **kw)
        if rank == 1 and step_no[0] == 2:
            net.sa1.mlp[0].gp("W").view(-1)[3] = float("nan")
        return out
    net.sa1.backward = poisoned_sa1
    cot = dict(proposals_output=torch.zeros(B, 256, 79), votes_xyz=None)
    flats, states = [], []
    for step in (1, 2, 3):
        step_no[0] = step
        net.train_step(torch.zeros(B, 64, 3), cot, world)
        flats.append(net.store.flat.numpy().copy())
        states.append(guard.read())
    q.put((rank, flats, states, net._step, bool(np.isfinite(net._m.numpy()).all())))
    dist.barrier()
    dist.destroy_process_group()


def test_a_gradient_poisoned_on_one_rank_is_skipped_on_both():
    from test_dp_gloo import _free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_guard_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=180) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    (_, f0, s0, n0, ok0), (_, f1, s1, n1, ok1) = res
    for a, b in zip(f0, f1):
        assert (a.view(np.int32) == b.view(np.int32)).all()           # the replicas stay identical, step by step
    assert s0 == s1 and n0 == n1 == 3 and ok0 and ok1
    assert (f0[1].view(np.int32) == f0[0].view(np.int32)).all()       # step 2 was skipped on BOTH ranks, rank 0's clean gradient included
    assert not (f0[2] == f0[1]).all() and np.isfinite(f0[2]).all()    # step 3 trains again
    assert [s["skipped"] for s in s0] == [0, 1, 1] and [s["consecutive"] for s in s0] == [0, 1, 0]
    assert s0[2]["seen"] == 3 and s0[2]["last_skip_step"] == 2
