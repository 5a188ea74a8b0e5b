"""Host side of networks/head_base.py: the draw order of the seeded initialisation of MaskHead, BoxHead and RPNHead, restated
here call by call, and the parameter methods the three heads inherit, under one set of assertions -- no GPU needed."""
import pytest
import torch

from apse_uav_amd.networks.box_head import BoxHead, merge_box_head
from apse_uav_amd.networks.mask_head import MaskHead, merge_full_mask_rcnn
from apse_uav_amd.networks.rpn_head import RPNHead, merge_rpn_head

K = 2
MASK_SHAPES = {}
for _i in range(1, 5):
    MASK_SHAPES["mask_fcn%d.weight" % _i] = (256, 256, 3, 3)
    MASK_SHAPES["mask_fcn%d.bias" % _i] = (256,)
MASK_SHAPES.update({"deconv.weight": (256, 256, 2, 2), "deconv.bias": (256,), "predictor.weight": (K, 256, 1, 1), "predictor.bias": (K,)})
RPN_SHAPES = {"conv.weight": (256, 256, 3, 3), "conv.bias": (256,), "objectness_logits.weight": (3, 256, 1, 1),
              "objectness_logits.bias": (3,), "anchor_deltas.weight": (12, 256, 1, 1), "anchor_deltas.bias": (12,)}


def box_shapes(k):
    return {"box_head.fc1.weight": (1024, 12544), "box_head.fc1.bias": (1024,), "box_head.fc2.weight": (1024, 1024),
            "box_head.fc2.bias": (1024,), "box_predictor.cls_score.weight": (k + 1, 1024), "box_predictor.cls_score.bias": (k + 1,),
            "box_predictor.bbox_pred.weight": (4 * k, 1024), "box_predictor.bbox_pred.bias": (4 * k,)}


def mask_weight(name, t):
    if name.startswith("predictor"):
        torch.nn.init.normal_(t, std=0.001)
    else:
        torch.nn.init.kaiming_normal_(t, mode="fan_out", nonlinearity="relu")


def box_weight(name, t):
    if name.startswith("box_head"):
        torch.nn.init.kaiming_uniform_(t, a=1)
    elif "cls_score" in name:
        torch.nn.init.normal_(t, std=0.01)
    else:
        torch.nn.init.normal_(t, std=0.001)


def rpn_weight(name, t):
    torch.nn.init.normal_(t, std=0.01)


def restated(shapes, weight, seed):
    """The rule: one pass over the names in order, a zeroed CPU tensor each, the in-place init on the weights only."""
    torch.manual_seed(seed)
    out = {}
    for name, shape in shapes.items():
        t = torch.zeros(shape)
        if name.endswith(".weight"):
            weight(name, t)
        out[name] = t
    return out


HEADS = {
    "mask": (lambda: MaskHead(K, "cpu"), MASK_SHAPES, mask_weight, merge_full_mask_rcnn, "mask-head"),
    "box": (lambda: BoxHead(K, "cpu"), box_shapes(K), box_weight, merge_box_head, "box-head"),
    "rpn": (lambda: RPNHead("cpu"), RPN_SHAPES, rpn_weight, merge_rpn_head, "RPN-head"),
}


@pytest.mark.parametrize("kind", list(HEADS))
def test_seeded_initialisation_is_the_restated_draw_order(kind):
    make, shapes, weight, _, _ = HEADS[kind]
    want = restated(shapes, weight, 5)
    torch.manual_seed(5)
    got = make().state_dict()
    assert list(got) == list(shapes)
    for name in shapes:
        assert got[name].dtype == torch.float32 and torch.equal(got[name], want[name]), name
        assert name.endswith(".weight") == bool(got[name].abs().max() > 0), name


def test_keep_predictor_draws_all_eight_then_overwrites_fc():
    src = restated(box_shapes(K), box_weight, 9)
    want = restated(box_shapes(3), box_weight, 5)               # the predictor tensors are draws 5 .. 8 of this sequence
    torch.manual_seed(5)
    head = BoxHead(3, "cpu")
    assert head.load_state_dict(src, keep_predictor=True) == []
    got = head.state_dict()
    for name in got:
        assert torch.equal(got[name], src[name] if name.startswith("box_head") else want[name]), name
    # on a head that already has parameters nothing is drawn and the predictor stays
    src2 = restated(box_shapes(K), box_weight, 11)
    before = torch.random.get_rng_state()
    head.load_state_dict(src2, keep_predictor=True)
    assert torch.equal(torch.random.get_rng_state(), before)
    assert torch.equal(head.state_dict()["box_predictor.bbox_pred.weight"], want["box_predictor.bbox_pred.weight"])
    assert not torch.equal(head.state_dict()["box_head.fc2.weight"], src["box_head.fc2.weight"])


def _filled(shapes, base=1.0):
    return {name: torch.full(shape, base + i) for i, (name, shape) in enumerate(shapes.items())}


@pytest.mark.parametrize("kind", list(HEADS))
def test_shared_parameter_methods(kind):
    make, shapes, _, merge, noun = HEADS[kind]
    names = list(shapes)
    sd = _filled(shapes)
    head = make()
    assert head.load_state_dict(sd) == []                      # no draw: loading into a fresh head starts from zeros
    params = list(head.parameters())
    assert [n for n, _ in head.named_parameters()] == names
    assert all(p.is_leaf and p.requires_grad and p.dtype == torch.float32 for p in params)
    # state_dict: detached clones in name order; the round trip, bare and prefixed
    got = head.state_dict()
    assert list(got) == names and all(torch.equal(got[n], sd[n]) and not got[n].requires_grad for n in names)
    assert all(got[n].data_ptr() != p.data_ptr() for n, p in head.named_parameters())
    prefixed = head.state_dict(head.prefix)
    assert list(prefixed) == [head.prefix + n for n in names]
    other = make()
    other.load_state_dict(dict(prefixed, **{"backbone.x": torch.ones(1)}))
    assert all(torch.equal(a, b) for a, b in zip(other.state_dict().values(), got.values()))
    # a missing key
    short = {n: v for n, v in sd.items() if n != names[-1]}
    with pytest.raises(RuntimeError, match="missing %s keys: %s" % (noun, names[-1])):
        make().load_state_dict(short)
    assert make().load_state_dict(short, strict=False) == [names[-1]]
    # a shape mismatch
    with pytest.raises(RuntimeError, match="size mismatch for %s" % names[0]):
        make().load_state_dict(dict(sd, **{names[0]: torch.zeros(3)}))
    # zero_grad, both modes
    for p in params:
        p.grad = torch.ones_like(p)
    grads = [p.grad for p in params]
    head.zero_grad(set_to_none=False)
    assert all(p.grad is g and float(g.abs().max()) == 0.0 for p, g in zip(params, grads))
    head.zero_grad()
    assert all(p.grad is None for p in params)
    # to: the same leaves, their gradients kept
    params[0].grad = torch.ones_like(params[0])
    assert head.to("cpu") is head
    after = list(head.parameters())
    assert all(a is b and a.is_leaf and a.requires_grad for a, b in zip(after, params))
    assert torch.equal(after[0].grad, torch.ones_like(after[0])) and after[1].grad is None
    assert head.eval() is head and not head.training and head.train().training
    # merging into a detector state
    det = {"backbone.x": torch.ones(1), "model.pixel_mean": torch.ones(3), head.prefix + names[0]: torch.zeros(shapes[names[0]])}
    merged = merge(det, got)
    assert set(merged) == {"backbone.x", "pixel_mean"} | {head.prefix + n for n in names}
    assert all(torch.equal(merged[head.prefix + n], sd[n]) for n in names)                   # the trained head wins
    again = merge(det, {"model." + k: v for k, v in prefixed.items()})
    assert all(torch.equal(merged[k], again[k]) for k in merged)
    assert set(merge(det, dict(got, **{"backbone.y": torch.ones(1)}))) == set(merged)        # a detector's other keys pass
    with pytest.raises(KeyError, match="%s: 'stray' is not an? %s parameter" % (merge.__name__, noun)):
        merge(det, dict(got, stray=torch.ones(1)))
    with pytest.raises(KeyError, match="%s: the %s state has %d of %d parameters" % (merge.__name__, noun, len(names) - 1, len(names))):
        merge(det, short)
