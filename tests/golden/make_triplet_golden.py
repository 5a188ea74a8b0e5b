#!/usr/bin/env python3
"""Generate the association-head training golden (build container only): tests/golden/triplet_golden.npz.

Run from the repo root:  python tests/golden/make_triplet_golden.py
Needs /root/reference (read-only); only the .npz this script writes is committed.

What is imported from the reference, run with CPU torch autograd:
  dcnn/online_triplet_loss/losses.py     batch_hard_triplet_loss, batch_all_triplet_loss (pure torch; its debug print is
                                         silenced while it runs)
  dcnn/networks/association_head.py      AssociationHead (pure torch)
Contents (keys prefixed by the case name):
  loss cases: labels, embeddings (D = 32, unit rows), and for hard / all x squared 0 / 1: loss, dE (and frac for all).
    Seeded n = 2, 7, 48, 300 plus structural cases: a label with one member, a single label, an anchor whose only negative
    is its row maximum, n = 1, duplicate embeddings.
  traj_*: 5 steps of train_association_head.py's loop on AssociationHead(roi_size=2, input_depth=16): closed-form initial
    weights and RoIs (make_golden.formula_tensor), batch_hard_triplet_loss(margin=0.2), torch.optim.SGD(lr=0.01,
    momentum=0.9); per-step losses, the final fc.bias and fc.weight @ a closed-form projection [K][8].
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import formula_tensor  # noqa: E402

D = 32


def loss_cases():
    g = torch.Generator().manual_seed(20)
    cases = {}
    for n in (2, 7, 48, 300):
        lab = torch.randint(0, max(2, n // 6), (n,), generator=g).double() + 1000.0
        e = torch.nn.functional.normalize(torch.randn(n, D, generator=g), dim=1)
        cases["seed%d" % n] = (lab, e)
    e = torch.nn.functional.normalize(torch.randn(9, D, generator=g), dim=1)
    cases["lonely"] = (torch.tensor([1005., 1005., 1005., 2001., 2001., 2001., 2001., 1007., 1005.]), e)   # 1007: no positive
    cases["one_label"] = (torch.full((6,), 1001.0), torch.nn.functional.normalize(torch.randn(6, D, generator=g), dim=1))
    # anchor 0: its only negative (row 4) is the farthest row: the hardest negative value ties with the diagonal's
    base = torch.zeros(5, D)
    base[0, 0] = 1.0
    base[1] = torch.nn.functional.normalize(torch.tensor([1.0, 0.3] + [0.0] * (D - 2)), dim=0)
    base[2] = torch.nn.functional.normalize(torch.tensor([1.0, -0.4] + [0.0] * (D - 2)), dim=0)
    base[3] = torch.nn.functional.normalize(torch.tensor([0.9, 0.1, 0.2] + [0.0] * (D - 3)), dim=0)
    base[4] = torch.nn.functional.normalize(torch.tensor([1.0, 0.45] + [0.0] * (D - 2)), dim=0)   # just past the positives
    cases["neg_is_rowmax"] = (torch.tensor([7., 7., 7., 7., 9.]), base)
    cases["n1"] = (torch.tensor([3.0]), torch.nn.functional.normalize(torch.randn(1, D, generator=g), dim=1))
    e = torch.nn.functional.normalize(torch.randn(8, D, generator=g), dim=1)
    e[3] = e[1]
    e[5] = e[1]
    e[6] = e[2]
    cases["dups"] = (torch.tensor([1., 1., 2., 1., 2., 1., 3., 3.]), e)
    return cases


def traj_inputs():
    K = 16 * 2 * 2
    w0 = formula_tensor((128, K), 29, 13, 211, 2048.0)
    b0 = formula_tensor((128,), 7, 3, 41, 256.0)
    xs = [formula_tensor((12, 16, 2, 2), 31 + s, 17, 307, 64.0) for s in range(5)]
    ids = [torch.tensor([float(1000 + (i * (s + 3)) % 4) for i in range(12)]) for s in range(5)]
    proj = formula_tensor((K, 8), 11, 5, 97, 32.0)
    return w0, b0, xs, ids, proj


def main():
    sys.path.insert(0, os.path.join(REF, "dcnn"))
    from online_triplet_loss.losses import batch_all_triplet_loss, batch_hard_triplet_loss
    from networks.association_head import AssociationHead

    out = {}
    for name, (lab, e) in loss_cases().items():
        out[name + "_labels"] = lab.numpy().astype(np.float64)
        out[name + "_emb"] = e.numpy().astype(np.float32)
        for sq in (0, 1):
            x = e.clone().requires_grad_(True)
            loss = batch_hard_triplet_loss(lab, x, 0.2, squared=bool(sq))
            loss.backward()
            out["%s_hard_sq%d_loss" % (name, sq)] = np.float32(loss.item())
            out["%s_hard_sq%d_dE" % (name, sq)] = x.grad.numpy().astype(np.float32)
            x = e.clone().requires_grad_(True)
            with contextlib.redirect_stdout(io.StringIO()):
                loss, frac = batch_all_triplet_loss(lab, x, 0.2, squared=bool(sq))
            loss.backward()
            out["%s_all_sq%d_loss" % (name, sq)] = np.float32(loss.item())
            out["%s_all_sq%d_frac" % (name, sq)] = np.float32(float(frac))
            out["%s_all_sq%d_dE" % (name, sq)] = x.grad.numpy().astype(np.float32)

    w0, b0, xs, ids, proj = traj_inputs()
    head = AssociationHead(roi_size=2, input_depth=16)
    head.load_state_dict({"fc.weight": w0, "fc.bias": b0})
    opt = torch.optim.SGD(head.parameters(), lr=0.01, momentum=0.9)
    losses = []
    for s in range(5):
        opt.zero_grad()
        emb = head(xs[s])
        loss = batch_hard_triplet_loss(ids[s], emb, margin=0.2, device="cpu")
        loss.backward()
        opt.step()
        losses.append(loss.item())
    out["traj_losses"] = np.array(losses, np.float32)
    out["traj_bias"] = head.fc.bias.detach().numpy().astype(np.float32)
    out["traj_wproj"] = (head.fc.weight.detach() @ proj).numpy().astype(np.float32)
    path = os.path.join(HERE, "triplet_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
