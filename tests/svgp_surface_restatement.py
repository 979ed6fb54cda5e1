"""torch fp64 restatement of the point-cloud surface SVGP's training objective (gpt_svgp_surface_train; reference:
policy_transportation/models/torch/stocastic_variational_gaussian_process.py:15-89): the objective of
tests/svgp_elbo_restatement.py with a length-scale per task, raw_ls (T,D).  Test helper only: the product package never
imports it.  Gradients come from torch.autograd."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.svgp_elbo_restatement import JITTER, NOISE_FLOOR, PARAM_NAMES, kl_numpy, rbf, to_torch  # noqa: F401


def init_params(X, Y, idx):
    """The surface model's initialisation: Z = X[idx], m = 0, C = I, every raw hyper-parameter 0 (raw_ls (T,D))."""
    X = np.asarray(X, np.float64)
    Zn, T, D = len(idx), np.asarray(Y).shape[1], X.shape[1]
    return {"Z": X[idx].copy(), "m": np.zeros((T, Zn)), "C": np.tile(np.eye(Zn), (T, 1, 1)),
            "raw_ls": np.zeros((T, D)), "raw_os": np.zeros(T), "raw_noise": np.zeros(T + 1)}


def loss(p, Xb, Yb, num_data):
    """Negative ELBO of one minibatch (Xb (b,D), Yb (b,T)), as a 0-d tensor."""
    Z, m, C = p["Z"], p["m"], p["C"]
    Zn, T, b = Z.shape[0], m.shape[0], Xb.shape[0]
    ls = F.softplus(p["raw_ls"])
    c = F.softplus(p["raw_os"])
    noise = (NOISE_FLOOR + F.softplus(p["raw_noise"][:T])) + (NOISE_FLOOR + F.softplus(p["raw_noise"][T]))
    eye = torch.eye(Zn, dtype=Z.dtype, device=Z.device)
    total = Z.new_zeros(())
    for t in range(T):
        L = torch.linalg.cholesky(c[t] * rbf(Z, Z, ls[t]) + JITTER * eye)
        A = torch.linalg.solve_triangular(L, c[t] * rbf(Z, Xb, ls[t]), upper=False)
        Ct = torch.tril(C[t])
        S = Ct @ Ct.T
        mu = A.T @ m[t]
        v = c[t] + JITTER + ((S - eye) @ A * A).sum(0)
        lik = -0.5 * torch.log(2 * math.pi * noise[t]) - ((Yb[:, t] - mu) ** 2 + v) / (2 * noise[t])
        kl = 0.5 * (torch.trace(S) + m[t] @ m[t] - Zn - torch.log(torch.diagonal(Ct) ** 2).sum())
        total = total - lik.sum() / b + kl / num_data
    return total


def loss_and_grad(p, Xb, Yb, num_data):
    """(loss, {name: gradient}) as numpy float64."""
    tp = to_torch(p, requires_grad=True)
    val = loss(tp, torch.as_tensor(np.asarray(Xb, np.float64)), torch.as_tensor(np.asarray(Yb, np.float64)), num_data)
    val.backward()
    return float(val.detach()), {k: tp[k].grad.numpy().copy() for k in PARAM_NAMES}


def adam_train(p, X, Y, idx, batch_begin, lr=0.01, n_steps=None, device="cpu"):
    """torch.optim.Adam (lr, betas (0.9, 0.999), eps 1e-8) over every parameter on the schedule X[idx[bb[s]:bb[s+1]]]
    (the first n_steps steps); returns (parameters, per-step losses)."""
    tp = to_torch(p, requires_grad=True, device=device)
    X = torch.as_tensor(np.asarray(X, np.float64), device=device)
    Y = torch.as_tensor(np.asarray(Y, np.float64), device=device)
    opt = torch.optim.Adam([tp[k] for k in PARAM_NAMES], lr=lr, betas=(0.9, 0.999), eps=1e-8, foreach=False)
    trace = []
    steps = len(batch_begin) - 1 if n_steps is None else n_steps
    for s in range(steps):
        rows = torch.as_tensor(np.asarray(idx[batch_begin[s]:batch_begin[s + 1]], np.int64), device=device)
        opt.zero_grad()
        val = loss(tp, X[rows], Y[rows], X.shape[0])
        val.backward()
        opt.step()
        trace.append(float(val.detach()))
    return {k: tp[k].detach().cpu().numpy().copy() for k in PARAM_NAMES}, np.array(trace)
