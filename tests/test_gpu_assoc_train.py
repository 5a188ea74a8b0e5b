"""-m gpu: association-head training kernels (csrc/assoc_train.hip) against the reference's golden
(tests/golden/make_triplet_golden.py), the numpy restatement (tests/assoc_train_ref.py), CPU autograd and torch.optim.SGD."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import assoc_train_ref as R  # noqa: E402

CASES = ["seed2", "seed7", "seed48", "seed300", "lonely", "one_label", "neg_is_rowmax", "n1", "dups"]


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "triplet_golden.npz"))


def _grad_ok(got, ref):
    scale = max(float(np.abs(ref).max()), 1e-30)
    return float(np.abs(got - ref).max()) <= 1e-4 * scale + 1e-12


def _hip_loss(kind, lab, e, squared):
    from apse_uav_amd.online_triplet_loss import batch_all_triplet_loss, batch_hard_triplet_loss
    x = torch.from_numpy(e).cuda().requires_grad_(True)
    labels = torch.from_numpy(lab).cuda()
    if kind == "hard":
        loss = batch_hard_triplet_loss(labels, x, 0.2, squared=bool(squared), device="cuda:0")
        frac = None
    else:
        loss, frac = batch_all_triplet_loss(labels, x, 0.2, squared=bool(squared))
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), (None if frac is None else float(frac)), x.grad.cpu().numpy()


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("squared", [0, 1])
def test_losses_against_golden_and_restatement(gold, case, squared):
    lab, e = gold[case + "_labels"], gold[case + "_emb"]
    loss, _, de = _hip_loss("hard", lab, e, squared)
    gl = float(gold["%s_hard_sq%d_loss" % (case, squared)])
    assert loss == pytest.approx(gl, rel=1e-5, abs=1e-7)
    assert _grad_ok(de, gold["%s_hard_sq%d_dE" % (case, squared)])
    rl, rde = R.batch_hard(lab, e, 0.2, squared)
    assert loss == pytest.approx(float(rl), rel=1e-5, abs=1e-7) and _grad_ok(de, rde)
    loss, frac, de = _hip_loss("all", lab, e, squared)
    assert loss == pytest.approx(float(gold["%s_all_sq%d_loss" % (case, squared)]), rel=1e-5, abs=1e-7)
    assert frac == pytest.approx(float(gold["%s_all_sq%d_frac" % (case, squared)]), rel=1e-6)
    assert _grad_ok(de, gold["%s_all_sq%d_dE" % (case, squared)])


def test_empty_and_single():
    from apse_uav_amd.online_triplet_loss import batch_all_triplet_loss, batch_hard_triplet_loss
    x = torch.zeros((0, 128), device="cuda", requires_grad=True)
    loss = batch_hard_triplet_loss(torch.zeros(0, device="cuda"), x, 0.2)
    assert torch.isnan(loss.cpu())
    la, fr = batch_all_triplet_loss(torch.zeros(0, device="cuda"), x, 0.2)
    assert float(la) == 0.0 and float(fr) == 0.0
    x = torch.nn.functional.normalize(torch.randn(1, 128), dim=1).cuda().requires_grad_(True)
    loss = batch_hard_triplet_loss(torch.tensor([5.0], device="cuda"), x, 0.2)
    loss.backward()
    assert float(loss) == pytest.approx(0.2) and not x.grad.cpu().any()


def _head(roi, depth, seed):
    from apse_uav_amd.networks.association_head import AssociationHead
    g = torch.Generator().manual_seed(seed)
    head = AssociationHead(roi_size=roi, input_depth=depth)
    k = depth * roi * roi
    head.load_state_dict({"fc.weight": torch.randn(128, k, generator=g) / k ** 0.5, "fc.bias": torch.randn(128, generator=g) * 0.1})
    return head.to("cuda")


def test_fc_forward_matches_inference_path():
    head = _head(10, 256, 1)
    x = torch.randn(37, 256, 10, 10, generator=torch.Generator().manual_seed(2)).cuda()
    ref = head(x).cpu()                                    # inference: apse_conv2d + apse_l2_normalize
    head.train()
    with torch.no_grad():
        got = head(x).cpu()
    assert float((got - ref).abs().max()) < 1e-5
    head.eval()
    again = head(x).cpu()
    assert torch.equal(again, ref)                          # bit-identical after a train()/eval() round trip


def test_fc_backward_matches_autograd():
    head = _head(4, 32, 3)
    x = torch.randn(21, 32, 4, 4, generator=torch.Generator().manual_seed(4))
    ge = torch.randn(21, 128, generator=torch.Generator().manual_seed(5))
    w = head.fc.weight.clone().requires_grad_(True)
    b = head.fc.bias.clone().requires_grad_(True)
    e = torch.nn.functional.normalize(torch.nn.functional.linear(x.view(21, -1), w, b), p=2, dim=1)
    (e * ge).sum().backward()
    head.train()
    out = head(x.cuda())
    assert float((out.detach().cpu() - e.detach()).abs().max()) < 1e-5
    (out * ge.cuda()).sum().backward()
    gw, gb = head.fc.weight.grad.cpu(), head.fc.bias.grad.cpu()
    assert float((gw - w.grad).abs().max()) <= 1e-4 * float(w.grad.abs().max())
    assert float((gb - b.grad).abs().max()) <= 1e-4 * float(b.grad.abs().max())
    # a second backward accumulates into .grad, as autograd does on a leaf
    out2 = head(x.cuda())
    (out2 * ge.cuda()).sum().backward()
    assert float((head.fc.bias.grad.cpu() - 2 * b.grad).abs().max()) <= 2e-4 * float(b.grad.abs().max())


def test_sgd_matches_torch():
    from apse_uav_amd.optim import SGD
    g = torch.Generator().manual_seed(6)
    for kw in (dict(lr=0.01, momentum=0.9), dict(lr=0.05), dict(lr=0.02, momentum=0.8, dampening=0.1, weight_decay=1e-3),
               dict(lr=0.03, momentum=0.7, nesterov=True, weight_decay=0.01)):
        p0 = torch.randn(1000, 3, generator=g)
        grads = [torch.randn(1000, 3, generator=g) for _ in range(5)]
        a = p0.clone().cuda().requires_grad_(True)
        b = p0.clone().cuda().requires_grad_(True)
        oa, ob = SGD([a], **kw), torch.optim.SGD([b], **kw)
        for s in range(5):
            oa.zero_grad()
            ob.zero_grad()
            a.grad = grads[s].cuda()
            b.grad = grads[s].cuda()
            oa.step()
            ob.step()
        torch.cuda.synchronize()
        assert float((a.detach() - b.detach()).abs().max()) <= 1e-6 * float(b.detach().abs().max()), kw


def _trajectory(opt_cls):
    from make_triplet_golden import traj_inputs
    from apse_uav_amd.networks.association_head import AssociationHead
    from apse_uav_amd.online_triplet_loss import batch_hard_triplet_loss
    w0, b0, xs, ids, proj = traj_inputs()
    head = AssociationHead(roi_size=2, input_depth=16)
    head.load_state_dict({"fc.weight": w0, "fc.bias": b0})
    head.to(torch.device("cuda:0"))
    head.train()
    opt = opt_cls(head.parameters(), lr=0.01, momentum=0.9)
    losses = []
    for s in range(5):
        opt.zero_grad()
        emb = head(xs[s].cuda())
        loss = batch_hard_triplet_loss(ids[s].cuda(), emb, margin=0.2, device="cuda:0")
        loss.backward()
        opt.step()
        losses.append(loss.item())
    sd = head.state_dict()
    return np.array(losses, np.float32), sd["fc.bias"].cpu().numpy(), sd["fc.weight"].cpu().numpy(), proj.numpy()


def test_trajectory_against_golden(gold):
    from apse_uav_amd.optim import SGD
    for opt_cls in (SGD, torch.optim.SGD):
        losses, bias, w, proj = _trajectory(opt_cls)
        np.testing.assert_allclose(losses, gold["traj_losses"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(bias, gold["traj_bias"], rtol=0, atol=1e-5)
        np.testing.assert_allclose(w @ proj, gold["traj_wproj"], rtol=0, atol=1e-4)


def test_bit_identical_runs():
    from apse_uav_amd.optim import SGD
    a = _trajectory(SGD)
    b = _trajectory(SGD)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    # a large batch through the split-K forward and the per-anchor kernels
    from apse_uav_amd.online_triplet_loss import batch_all_triplet_loss, batch_hard_triplet_loss
    g = torch.Generator().manual_seed(8)
    e = torch.nn.functional.normalize(torch.randn(600, 128, generator=g), dim=1).cuda()
    lab = (torch.randint(0, 60, (600,), generator=g).double() + 1000).cuda()
    outs = []
    for _ in range(2):
        r = []
        for fn in (batch_hard_triplet_loss, lambda l, x, m: batch_all_triplet_loss(l, x, m)[0]):
            x = e.clone().requires_grad_(True)
            loss = fn(lab, x, 0.2)
            loss.backward()
            r += [loss.detach().cpu(), x.grad.cpu()]
        outs.append(r)
    assert all(torch.equal(p, q) for p, q in zip(*outs))


def test_limits_refused():
    from apse_uav_amd import _lib
    from apse_uav_amd.online_triplet_loss import batch_hard_triplet_loss
    lib = _lib.load()
    with pytest.raises(_lib.ApseError, match="2048"):
        batch_hard_triplet_loss(torch.zeros(2049, device="cuda"), torch.zeros(2049, 8, device="cuda"), 0.2)
    with pytest.raises(_lib.ApseError, match="D <= 256"):
        batch_hard_triplet_loss(torch.zeros(4, device="cuda"), torch.zeros(4, 257, device="cuda"), 0.2)
    assert lib.apse_assoc_fc_workspace_bytes(2049, 25600, 128) == 0
    assert lib.apse_assoc_fc_workspace_bytes(16, 256 * 32 * 32 + 1, 128) == 0
    assert lib.apse_assoc_fc_workspace_bytes(16, 25600, 257) == 0
    rc = lib.apse_assoc_fc_forward(None, None, None, 3000, 100, 128, None, None, None, 0, _lib.stream_ptr())
    assert rc == -1 and b"2048" in lib.apse_last_error(None)
    rc = lib.apse_sgd_step(None, None, None, 4, 0.1, 0.0, 0.1, 0.0, 1, 1, _lib.stream_ptr())
    assert rc == -1
