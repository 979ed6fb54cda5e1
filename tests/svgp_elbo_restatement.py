"""torch fp64 restatement of the SVGP training objective the variational-training path reproduces (reference:
policy_transportation/models/torch/stocastic_variational_gaussian_process_derivatives.py:15-63 model, :155-187 fit;
gpytorch's whitened VariationalStrategy, CholeskyVariationalDistribution, MultitaskGaussianLikelihood (rank 0) and
VariationalELBO as read, constants unpinned: gpytorch is not available).  Test helper only: the product package never
imports it.  Gradients come from torch.autograd.

Parameters (dict of float64 tensors / arrays):
  Z (Z,D) inducing points, m (T,Z) whitened variational means, C (T,Z,Z) variational Cholesky factors (lower triangle
  used), raw_ls (D,), raw_os (T,), raw_noise (T+1,) = per-task raw noises then the global one."""
import math

import numpy as np
import torch
import torch.nn.functional as F

JITTER = 1e-4          # gpytorch's float32 Cholesky jitter
NOISE_FLOOR = 1e-4     # GreaterThan(1e-4) on each likelihood noise
PARAM_NAMES = ("Z", "m", "C", "raw_ls", "raw_os", "raw_noise")


def init_params(X, Y, idx):
    """The reference's initialisation: Z = X[idx], m_t = Y[idx, t], C_t = I, every raw hyper-parameter 0."""
    X = np.asarray(X, np.float64)
    Y = np.asarray(Y, np.float64)
    Zn, T, D = len(idx), Y.shape[1], X.shape[1]
    return {"Z": X[idx].copy(), "m": Y[idx].T.copy(), "C": np.tile(np.eye(Zn), (T, 1, 1)),
            "raw_ls": np.zeros(D), "raw_os": np.zeros(T), "raw_noise": np.zeros(T + 1)}


def rbf(a, b, ls):
    d = (a[:, None, :] - b[None, :, :]) / ls
    return torch.exp(-0.5 * (d * d).sum(-1))


def loss(p, Xb, Yb, num_data):
    """Negative ELBO of one minibatch (Xb (b,D), Yb (b,T)), as a 0-d tensor."""
    Z, m, C = p["Z"], p["m"], p["C"]
    Zn, T, b = Z.shape[0], m.shape[0], Xb.shape[0]
    ls = F.softplus(p["raw_ls"])
    c = F.softplus(p["raw_os"])
    noise = (NOISE_FLOOR + F.softplus(p["raw_noise"][:T])) + (NOISE_FLOOR + F.softplus(p["raw_noise"][T]))
    eye = torch.eye(Zn, dtype=Z.dtype, device=Z.device)
    Ruu, Rux = rbf(Z, Z, ls), rbf(Z, Xb, ls)
    total = Z.new_zeros(())
    for t in range(T):
        L = torch.linalg.cholesky(c[t] * Ruu + JITTER * eye)
        A = torch.linalg.solve_triangular(L, c[t] * Rux, upper=False)          # (Z,b)
        Ct = torch.tril(C[t])
        S = Ct @ Ct.T
        mu = A.T @ m[t]
        v = c[t] + JITTER + ((S - eye) @ A * A).sum(0)
        lik = -0.5 * torch.log(2 * math.pi * noise[t]) - ((Yb[:, t] - mu) ** 2 + v) / (2 * noise[t])
        kl = 0.5 * (torch.trace(S) + m[t] @ m[t] - Zn - torch.log(torch.diagonal(Ct) ** 2).sum())
        total = total - lik.sum() / b + kl / num_data
    return total


def to_torch(p, requires_grad=False, device="cpu"):
    return {k: torch.tensor(np.asarray(p[k], np.float64), requires_grad=requires_grad, device=device) for k in PARAM_NAMES}


def loss_and_grad(p, Xb, Yb, num_data):
    """(loss, {name: gradient}) as numpy float64."""
    tp = to_torch(p, requires_grad=True)
    val = loss(tp, torch.as_tensor(np.asarray(Xb, np.float64)), torch.as_tensor(np.asarray(Yb, np.float64)), num_data)
    val.backward()
    return float(val.detach()), {k: tp[k].grad.numpy().copy() for k in PARAM_NAMES}


def adam_train(p, X, Y, idx, batch_begin, lr=0.01):
    """torch.optim.Adam (lr, betas (0.9, 0.999), eps 1e-8) over every parameter on the schedule X[idx[bb[s]:bb[s+1]]];
    returns (parameters, per-step losses)."""
    tp = to_torch(p, requires_grad=True)
    X = torch.as_tensor(np.asarray(X, np.float64))
    Y = torch.as_tensor(np.asarray(Y, np.float64))
    opt = torch.optim.Adam([tp[k] for k in PARAM_NAMES], lr=lr, betas=(0.9, 0.999), eps=1e-8, foreach=False)
    trace = []
    for s in range(len(batch_begin) - 1):
        rows = torch.as_tensor(np.asarray(idx[batch_begin[s]:batch_begin[s + 1]], np.int64))
        opt.zero_grad()
        val = loss(tp, X[rows], Y[rows], X.shape[0])
        val.backward()
        opt.step()
        trace.append(float(val.detach()))
    return {k: tp[k].detach().numpy().copy() for k in PARAM_NAMES}, np.array(trace)


def kl_numpy(m, C):
    """KL(N(m, C C^T) || N(0, I)) in closed form (numpy, slogdet)."""
    Ct = np.tril(C)
    S = Ct @ Ct.T
    Zn = len(m)
    return 0.5 * (np.trace(S) + m @ m - Zn - np.linalg.slogdet(S)[1])


def whitened_predictive(p, x):
    """The SVGP predictive of the trained model at x (M,D): mean (M,T) = A^T m, variance (M,T) = c + eps + a^T (S - I) a."""
    with torch.no_grad():
        tp = to_torch(p)
        x = torch.as_tensor(np.asarray(x, np.float64))
        ls = F.softplus(tp["raw_ls"])
        c = F.softplus(tp["raw_os"])
        Zn, T = tp["Z"].shape[0], tp["m"].shape[0]
        eye = torch.eye(Zn, dtype=torch.float64)
        Ruu, Rux = rbf(tp["Z"], tp["Z"], ls), rbf(tp["Z"], x, ls)
        mean, var = [], []
        for t in range(T):
            L = torch.linalg.cholesky(c[t] * Ruu + JITTER * eye)
            A = torch.linalg.solve_triangular(L, c[t] * Rux, upper=False)
            Ct = torch.tril(tp["C"][t])
            mean.append(A.T @ tp["m"][t])
            var.append(c[t] + JITTER + ((Ct @ Ct.T - eye) @ A * A).sum(0))
        return torch.stack(mean, 1).numpy(), torch.stack(var, 1).numpy()
