"""CPU: the named records of the geometry hand-over (pointnet2.SAGeometry / FPGeometry and the first-layer rows they carry, the four
chain inputs of mlp_chain_forward) and the owner of a net's prefetch state (model.GeometryPrefetch as net._geometry)."""
import pytest
import torch

from votenet_amd import model as VM
from votenet_amd import pointnet2 as P


class _Layout:
    """Stand-in for mlp.HalfLayout: all a record asks of it is tensors()."""

    def __init__(self):
        self.mine = [torch.zeros(2), torch.zeros(3)]

    def tensors(self):
        return list(self.mine)


def _same(got, want):
    """Exactly these tensor objects, once each (order free)."""
    got = list(got)
    return len(got) == len(want) and sorted(map(id, got)) == sorted(map(id, want))


@pytest.mark.parametrize("with_inverse", [False, True])
@pytest.mark.parametrize("with_layout", [False, True])
@pytest.mark.parametrize("form", [None, "narrow", "assembled"])
def test_a_level_geometry_lists_exactly_its_tensors(form, with_layout, with_inverse):
    fps_idx, new_xyz, idx, cnt = (torch.zeros(4, dtype=torch.int32), torch.zeros(4, 3), torch.zeros(4, 2, dtype=torch.int32),
                                  torch.zeros(4, dtype=torch.int32))
    want = [fps_idx, new_xyz, idx, cnt]
    if with_inverse:
        idx._inv = (torch.zeros(8, dtype=torch.int32), torch.zeros(5, dtype=torch.int32))
        want += list(idx._inv)
    half = _Layout() if with_layout else None
    first = None
    if form == "narrow":
        u8, mom = torch.zeros(8, 8), torch.zeros(72, dtype=torch.float64)
        first = P.NarrowRows(u8, mom, half) if with_layout else P.NarrowRows(u8, mom)
        want += [u8, mom]
    elif form == "assembled":
        geo, cntv, mom = torch.zeros(8, 4), torch.zeros(4, 4, dtype=torch.int64), torch.zeros(9, dtype=torch.float64)
        first = P.AssembledRows(geo, cntv, mom, half) if with_layout else P.AssembledRows(geo, cntv, mom)
        want += [geo, cntv, mom]
    if form is not None and with_layout:
        want += half.mine
    geom = P.SAGeometry(fps_idx, new_xyz, idx, cnt, first) if form is not None else P.SAGeometry(fps_idx, new_xyz, idx, cnt)
    assert geom.first is first and (first is None or first.half is half)
    assert _same(geom.tensors(), want)
    if first is not None:
        assert _same(first.tensors(), want[(6 if with_inverse else 4):])


@pytest.mark.parametrize("with_inverse", [False, True])
def test_the_interpolation_taps_list_exactly_their_tensors(with_inverse):
    idx, weight = torch.zeros(4, 3, dtype=torch.int32), torch.zeros(4, 3)
    want = [idx, weight]
    if with_inverse:
        idx._inv = (torch.zeros(12, dtype=torch.int32), torch.zeros(3, dtype=torch.int32))
        want += list(idx._inv)
    geom = P.FPGeometry(idx, weight)
    assert geom.idx is idx and geom.weight is weight and _same(geom.tensors(), want)


def test_the_four_chain_inputs_are_told_apart_by_type():
    t = torch.zeros(1)
    inputs = [P.DenseInput(t), P.GatherInput(t, t, None, t), P.NarrowInput(t, t), P.AssembledInput(t, t, t, t, t, t, t)]
    kinds = (P.DenseInput, P.GatherInput, P.NarrowInput, P.AssembledInput)
    for i, first in enumerate(inputs):
        assert [isinstance(first, k) for k in kinds] == [j == i for j in range(4)]
        assert P._FIRST_LAYERS[type(first)].__name__ == ("_first_dense", "_first_gather", "_first_narrow", "_first_assembled")[i]
    assert set(P._FIRST_LAYERS) == set(kinds)
    assert inputs[0].padded is None and inputs[2].half is None and inputs[3].half is None
    padded = torch.zeros(1, 4)
    assert P.DenseInput(padded[:, :3], padded).padded is padded
    layout = _Layout()
    assert P.NarrowInput(t, t, layout).half is layout and P.AssembledInput(t, t, t, t, t, t, t, layout).half is layout


def test_a_net_owns_one_prefetch_state_and_the_pool_keeps_its_identity():
    """tools/bench_legs.py empties the pool between legs through net.__dict__["_prefetched"]: that name must stay the pool itself."""
    cpu = torch.device("cpu")
    net = VM.VoteNetHotPath(cpu, seed=3, npoints=(64, 32, 16, 8))
    own = net._geometry
    assert isinstance(own, VM.GeometryPrefetch) and net.__dict__["_prefetched"] is own.pool
    assert (own.pool, own.rings, own.evictions, own.graphs_off, own.current, own.streams, own.turn) == ({}, {}, 0, False, None, None, 0)
    assert own.device == cpu and own.prop_npoint == net.proposal.npoint
    x = torch.zeros(2, 8, 3)
    own.pool[id(x)] = VM.PrefetchEntry(x, x._version, {}, {}, None, 0)
    own.rings["a shape"] = dict(graphs=[], turn=0, warm=1)
    own.current = object()
    entry = own.pool[id(x)]
    assert entry.x is x and (entry.graph, entry.generation, entry.feats, entry.feats_version) == (None, 0, None, 0)
    net.drop_graphs()
    assert net.__dict__["_prefetched"] is own.pool is net._geometry.pool and own.pool == {} and own.rings == {} and own.current is None
    assert net._geometry is own
