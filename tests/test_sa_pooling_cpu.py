"""CPU: the SAModule arguments of pointnet_sa_module it serves beyond the default (utils.py:93-158): `pooling` and `group_all` --
argument checks, parameter shapes, and the ABI entries of csrc/pool_modes.hip in the header and the library.  No compute launched."""
import pytest
import torch

from votenet_amd import pointnet2 as P


def _store():
    return P.ParamStore(torch.device("cpu"))


def test_unknown_pooling_is_a_value_error():
    with pytest.raises(ValueError, match="pooling"):
        P.SAModule(_store(), "sa", 64, 0.4, 16, 8, [32, 64], pooling="sum")
    with pytest.raises(ValueError):
        P.SAModule(_store(), "sa", 64, 0.4, 16, 8, [32, 64], pooling="MAX")


@pytest.mark.parametrize("pooling", ["max", "avg", "weighted_avg", "max_and_avg"])
def test_parameter_shapes_and_mlp2_width(pooling):
    s = _store()
    mod = P.SAModule(s, "sa", 64, 0.4, 16, 8, [32, 48], mlp2=[40, 24], pooling=pooling)
    s.materialize(0)
    assert s["sa/conv0/W"].shape == (3 + 8, 32) and s["sa/conv1/W"].shape == (32, 48)
    assert s["sa/conv1/gamma"].shape == (48,) and s["sa/conv1/beta"].shape == (48,)
    width = 96 if pooling == "max_and_avg" else 48  # [avg | max] (utils.py:143-146)
    assert s["sa/conv_post_0/W"].shape == (width, 40)
    assert s["sa/conv_post_1/W"].shape == (40, 24) and "sa/conv_post_1/gamma" not in s.views
    assert mod.pooling == pooling and mod.plain_pool == (pooling != "max")


def test_group_all_ignores_npoint_radius_nsample_and_knn():
    a, b = _store(), _store()
    ma = P.SAModule(a, "sa", 64, 0.4, 16, 8, [32, 64], group_all=True)
    mb = P.SAModule(b, "sa", 7, 123.0, 5, 8, [32, 64], knn=True, group_all=True)
    for m in (ma, mb):
        assert m.group_all and m.plain_pool and m.npoint == 1 and not m.knn
        assert m.radius is None and m.nsample is None
    a.materialize(0)
    b.materialize(0)
    assert [(n, s) for n, s, _ in a._specs] == [(n, s) for n, s, _ in b._specs]


def test_default_module_keeps_the_fused_forms():
    """pooling='max', group_all=False is today's module: the narrow / assembled / piece-layout forms stay eligible."""
    s = _store()
    sa1 = P.SAModule(s, "sa1", 2048, 0.2, 64, 3, [64, 64, 128], leaf=True)
    sa2 = P.SAModule(s, "sa2", 1024, 0.4, 64, 128, [128, 128, 256])
    avg1 = P.SAModule(s, "a1", 2048, 0.2, 64, 3, [64, 64, 128], leaf=True, pooling="avg")
    avg2 = P.SAModule(s, "a2", 1024, 0.4, 64, 128, [128, 128, 256], pooling="max_and_avg")
    all2 = P.SAModule(s, "g2", 1024, 0.4, 64, 128, [128, 128, 256], group_all=True)
    assert not sa1.plain_pool and not sa2.plain_pool
    for m in (avg1, avg2, all2):
        assert not m.narrow(8 * 2048 * 64) and not m.assembled(8, 20000) and not m.half_groups(8, 20000)


def test_pool_entries_are_declared_and_exported(hiplib):
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "votenet_hip.h")).read(), flags=re.S)
    for name in ("votenet_bn_relu_pool", "votenet_bn_relu_pool_workspace_floats", "votenet_sa_pool_weights", "votenet_sa_pool_grad",
                 "votenet_sa_pool_weights_grad"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(hiplib, name), name


def test_pool_workspace_query(hiplib):
    """Many small groups need no partials; a few huge ones (group_all) are split over workgroups."""
    assert hiplib.votenet_bn_relu_pool_workspace_floats(8 * 256, 16, 128) == 0
    ws = hiplib.votenet_bn_relu_pool_workspace_floats(8, 20480, 256)
    assert ws > 0 and ws % (3 * 8 * 256) == 0
    assert hiplib.votenet_bn_relu_pool_workspace_floats(0, 16, 128) == 0


def test_pool_entries_validate_arguments(hiplib):
    """Argument checks run before any launch: an unknown mode, k = 0, a missing weight vector."""
    from votenet_amd import _lib
    L = _lib.lib()
    assert L.votenet_bn_relu_pool(4, 16, 8, None, None, None, 1, 7, None, None, None, None, None) == 1
    assert b"mode" in L.votenet_last_error()
    assert L.votenet_bn_relu_pool(4, 0, 8, None, None, None, 1, 0, None, None, None, None, None) == 1
    assert L.votenet_bn_relu_pool(0, 16, 8, None, None, None, 1, 1, None, None, None, None, None) == 0  # groups == 0: nothing to do
    assert L.votenet_sa_pool_grad(4, 16, 8, -1, None, None, None, None, None) == 1
    assert L.votenet_sa_pool_grad(0, 16, 8, 2, None, None, None, None, None) == 0
    assert L.votenet_sa_pool_weights(2, 100, 2, 100, None, None, None, None, None) == 1  # group_all (no idx) takes m = 1
