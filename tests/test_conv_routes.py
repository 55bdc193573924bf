"""Conv2d.route (CPU): which kernels every convolution layer of the five benchmark configurations takes, against a table of
what the per-pass predicates that route replaced decided.

tests/golden/conv_routes.json was recorded from those predicates (Conv2d.x3_mode / fwd_on_xpw / halo_fwd / halo_dgrad /
planes_in / planes_dy / planes_wgrad, the storage answers, and SlotModel._forward_impl's split lists) with the same loops
as below: for every distinct layer geometry of `bench.make_args(bench.CONFIGS[n])`, n = 1..5, under x3 in {0, 15, 63, 127,
255} x planes in {0, 3} x precision in {fp32, bf16}:
  layers   [Cin, Cout, k, stride, pad, groups, bias, planes, x3, precision, forward families, input-gradient families,
            weight-gradient family, planes_in, planes_dy, x3_mode() truth]
  storage  [Cin, ..., bias, planes, precision, per map of `maps`: grad_storage, act_storage, planes_only(H, W, B),
            planes_only(H, W), dy_plane_only as 0 / 1]
  models   [config, precision, planes, x3, len(SlotModel._x3_convs), split items of a saving / non-saving forward as
            "layer:fd" (index among the model's non-stem Conv2d, forward planes, input-gradient planes), in launch order]
"""
import json
import os

import pytest

import bench
from scouter_amd.nn_hip import Conv2d, ConvRoute, StemConv2d
from scouter_amd.sloter.slot_model import SlotModel

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "conv_routes.json")
X3S, PLANES, PRECS = (0, 15, 63, 127, 255), (0, 3), ("fp32", "bf16")


def _geom(c):
    return [c.in_channels, c.out_channels, c.kernel_size, c.stride, c.padding, c.groups, c.bias is not None]


def _tables(maps):
    layers, storage, models = {}, {}, []
    for n in sorted(bench.CONFIGS):
        m = SlotModel(bench.make_args(bench.CONFIGS[n]))
        convs = [c for c in m.modules() if isinstance(c, Conv2d) and not isinstance(c, StemConv2d)]
        idx = {id(c): i for i, c in enumerate(convs)}
        for prec in PRECS:
            m.set_precision(prec)
            for planes in PLANES:
                m.set_planes(planes)
                for x3 in X3S:
                    m.set_x3(x3)
                    for c in convs:
                        r = c.route()
                        row = [",".join(r.fwd), ",".join(r.dgrad), r.wgrad, r.planes_in, r.planes_dy, int(bool(c.x3_mode()))]
                        assert layers.setdefault(tuple(_geom(c) + [c.planes, c.x3, c.precision]), row) == row
                        st = "".join("%d%d%d%d%d" % (c.grad_storage(*mp) is not None, c.act_storage(*mp) is not None,
                                                     c.planes_only(mp[1], mp[2], mp[0]), c.planes_only(mp[1], mp[2]),
                                                     c.dy_plane_only(*mp)) for mp in maps)
                        assert storage.setdefault(tuple(_geom(c) + [c.planes, c.precision]), st) == st
                    split = [" ".join("%d:%d%d" % (idx[id(c)], f, d) for c, f, d in m._split_items(save))
                             for save in (True, False)]
                    models.append([n, prec, planes, x3, len(m._x3_convs)] + split)
    return layers, storage, models


def test_routes_match_the_recorded_table():
    with open(GOLDEN) as f:
        want = json.load(f)
    layers, storage, models = _tables([tuple(mp) for mp in want["maps"]])
    assert [list(k) + v for k, v in sorted(layers.items())] == want["layers"]
    assert [list(k) + [v] for k, v in sorted(storage.items())] == want["storage"]
    assert models == want["models"]


@pytest.mark.parametrize("x3", (0, 127, 255))
def test_route_follows_a_direct_assignment(x3):
    """The route is cached on (x3, precision, planes): assigning a layer's switches after construction re-routes it."""
    c = Conv2d(32, 32, 3, 1, 1)
    assert c.route().dgrad == ()
    c.x3 = x3
    assert c.route().dgrad == (("xhalo",) if x3 & 64 else ())
    assert c.route().fwd == (("xhalo",) if x3 & 128 else ())
    c.precision = "bf16"
    assert c.route() == ConvRoute((), (), "igemm", False, False, 0, 0)
