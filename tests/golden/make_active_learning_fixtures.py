"""Writes tests/golden/active_learning_*.npz: the reference's greedy active-learning selection
(policy_transportation/models/gaussian_process_al.py:26-68) run by the reference's own class on small pools, with
fixed-bound kernels so that sklearn does not re-optimise theta between insertions.  Arrays only (allow_pickle=False).

Per case: pool X, targets Y, theta (c, length_scale, noise), alpha, seed (np.random.seed before fit), n_samples_max, the
kernel (nu: 0 = RBF), the reference's index sequence `selected` (rows of its self.X matched to the pool: initial subset,
then insertions), `selection_variance` (sklearn's std^2 of each inserted point, predicted by a regressor fitted on the
points before it), `min_gap` (below), and predict(return_std=True) / derivative(return_var=True) of the reference's
GaussianProcess (optimizer=None) fitted on the selected subset at 100 queries.  For the Matern case J / Jvar are the
reference's RBF formulas applied to a Matern k* (gaussian_process.py:63-102 does that for any kernel): recorded as the
reference returns them, but not a parity target — the package refuses those calls or, with matern_derivatives=True,
returns the analytic derivatives of the Matern posterior instead.

Near-ties.  The greedy rule is discontinuous: when the two largest variances agree to rounding, which point is taken is not
a property of the algorithm.  This generator therefore restates the selection as a pivoted Cholesky factorisation, follows
the reference's sequence with it and ASSERTS for every committed fixture that
  * at every insertion the relative gap between the largest and the second largest variance is >= MIN_GAP = 1e-7
    (about 1e8 x the fp64 rounding of these O(1) sums), and
  * at every insertion the largest variance lies strictly below the prior c + noise (no pool point sits at the saturated
    prior variance, where many points tie bit for bit).
Seeds and length-scales are searched until the reference meets both; a case that does not is not written.

usage: python tests/golden/make_active_learning_fixtures.py REFERENCE_ROOT"""
import contextlib
import importlib.util
import io
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MIN_GAP = 1e-7


def import_reference(ref_root):
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.modules.setdefault("Quaternion", types.ModuleType("Quaternion"))
    if ref_root not in sys.path:
        sys.path.insert(0, ref_root)
    spec = importlib.util.spec_from_file_location(
        "reference_gaussian_process_al", os.path.join(ref_root, "policy_transportation", "models", "gaussian_process_al.py"))
    al = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(al)
    al.tqdm = lambda it: it                       # no progress bar
    from policy_transportation.models.gaussian_process import GaussianProcess
    return al, GaussianProcess


def make_kernel(c, ls, noise, nu, bounds="fixed"):
    from sklearn.gaussian_process.kernels import RBF, Matern, WhiteKernel, ConstantKernel as C
    stat = RBF(ls, bounds) if nu == 0 else Matern(ls, bounds, nu=nu)
    return C(c, bounds) * stat + WhiteKernel(noise, bounds)


def kstat(h2, nu):
    """The stationary factor from squared scaled distances (sklearn/gaussian_process/kernels.py RBF, Matern)."""
    if nu == 0:
        return np.exp(-0.5 * h2)
    r = np.sqrt(h2)
    if nu == 0.5:
        return np.exp(-r)
    if nu == 1.5:
        return (1 + np.sqrt(3) * r) * np.exp(-np.sqrt(3) * r)
    return (1 + np.sqrt(5) * r + 5.0 / 3.0 * h2) * np.exp(-np.sqrt(5) * r)


def restatement(X, ls, c, noise, alpha, nu, n_initial, pivots):
    """Pivoted-Cholesky restatement following `pivots` (the first n_initial prescribed).  Returns the argmax the rule
    would have taken at each later step, d[p] at each step, and the relative top-two gap / largest variance there."""
    Xs = X / ls
    N, m = X.shape[0], len(pivots)
    P = np.zeros((N, m))
    d = np.full(N, c + noise)
    alive = np.ones(N, bool)
    choice, dsel, gaps, dmax = [], [], [], []
    for j, p in enumerate(pivots):
        if j >= n_initial:
            dd = np.where(alive, d, -np.inf)
            top = np.sort(dd)[-2:]
            choice.append(int(np.argmax(dd)))
            gaps.append((top[1] - top[0]) / top[1])
            dmax.append(top[1])
            dsel.append(d[p])
        col = (c * kstat(((Xs - Xs[p]) ** 2).sum(1), nu) - P[:, :j] @ P[p, :j]) / np.sqrt(d[p] + alpha)
        P[:, j] = col
        d = d - col ** 2
        alive[p] = False
    return np.array(choice), np.array(dsel), np.array(gaps), np.array(dmax)


def greedy_own(X, ls, c, noise, alpha, nu, initial, m):
    """The same rule choosing its own pivots (the cheap filter of the seed / length-scale search)."""
    Xs = X / ls
    N = X.shape[0]
    P = np.zeros((N, m))
    d = np.full(N, c + noise)
    alive = np.ones(N, bool)
    gap, sat = np.inf, False
    for j in range(m):
        if j < len(initial):
            p = int(initial[j])
        else:
            dd = np.where(alive, d, -np.inf)
            top = np.sort(dd)[-2:]
            p = int(np.argmax(dd))
            gap = min(gap, (top[1] - top[0]) / top[1])
            sat = sat or not top[1] < c + noise
        col = (c * kstat(((Xs - Xs[p]) ** 2).sum(1), nu) - P[:, :j] @ P[p, :j]) / np.sqrt(d[p] + alpha)
        P[:, j] = col
        d = d - col ** 2
        alive[p] = False
    return gap, sat


def draw_initial(seed, N, n_initial):
    np.random.seed(seed)
    return np.random.choice(range(N), size=n_initial, replace=False)      # the reference's draw (:31)


def build_case(al, RefGP, name, X, Y, Xq, c, noise, alpha, nu, m, ls_candidates, seeds):
    from sklearn.gaussian_process import GaussianProcessRegressor
    N, D = X.shape
    n_initial = int(0.1 * m)
    for ls in ls_candidates:
        ls = np.asarray(ls, np.float64)
        for seed in seeds:
            gap, sat = greedy_own(X, ls, c, noise, alpha, nu, draw_initial(seed, N, n_initial), m)
            if sat or gap < 2 * MIN_GAP:
                print(f"  {name}: ls {ls[0]:.4g} seed {seed}: min gap {gap:.2e}{' (saturated)' if sat else ''} - next")
                continue
            kern = make_kernel(c, ls, noise, nu)
            g = al.GaussianProcess(kern, alpha=alpha, n_samples_max=m)
            np.random.seed(seed)
            with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                g.fit(X, Y)
            selected = np.array([int(np.flatnonzero((X == r).all(1))[0]) for r in g.X], dtype=np.int64)
            assert len(set(selected.tolist())) == m and np.array_equal(X[selected], g.X) and np.array_equal(Y[selected], g.Y)
            choice, dsel, gaps, dmax = restatement(X, ls, c, noise, alpha, nu, n_initial, selected)
            assert np.array_equal(choice, selected[n_initial:]), f"{name}: the restatement leaves the reference's sequence"
            assert gaps.min() >= MIN_GAP, f"{name}: top-two gap {gaps.min():.3e} < {MIN_GAP:g}"
            assert (dmax < c + noise).all(), f"{name}: a pool point sits at the saturated prior variance"
            # the reference's std^2 at each insertion: sklearn's regressor on the points before it, as its loop has it
            selvar = np.zeros(m - n_initial)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                for t in range(n_initial, m):
                    gp = GaussianProcessRegressor(kernel=kern, alpha=alpha).fit(X[selected[:t]], Y[selected[:t]])
                    std = gp.predict(X[selected[t]][None, :], return_std=True)[1]
                    selvar[t - n_initial] = float(np.ravel(std)[0]) ** 2
            ref = RefGP(kernel=make_kernel(c, ls, noise, nu, bounds=(1e-5, 1e5)), alpha=alpha, optimizer=None)
            with contextlib.redirect_stdout(io.StringIO()):
                ref.fit(X[selected], Y[selected])
                mean, std = ref.predict(Xq, return_std=True)
                out = dict(mean=mean, std=std)
                out["J"], out["Jvar"] = ref.derivative(Xq, return_var=True)
            path = os.path.join(HERE, f"active_learning_{name}.npz")
            np.savez_compressed(path, X=X, Y=Y, Xq=Xq, constant_value=np.float64(c), length_scale=ls, noise_level=np.float64(noise),
                                alpha=np.float64(alpha), nu=np.float64(nu), seed=np.int64(seed), n_samples_max=np.int64(m),
                                n_initial=np.int64(n_initial), selected=selected, selection_variance=selvar,
                                min_gap=np.float64(gaps.min()), **out)
            print(f"active_learning_{name}.npz: pool {X.shape}, m {m}, ls {ls[0]:.4g}, seed {seed}, min gap {gaps.min():.3e}, "
                  f"max d/(c+noise) {dmax.max() / (c + noise):.4f}, {os.path.getsize(path)} bytes")
            return
    raise SystemExit(f"{name}: no seed / length-scale met the gap condition")


def uniform_pool(N, D, O, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, D))
    Y = (0.05 * np.sin(4 * X) + 0.01 * rng.standard_normal((N, D)))[:, :O]
    Xq = np.random.default_rng(seed + 100).uniform(-0.05, 1.05, (100, D))
    return X, Y, Xq


def main(ref_root):
    al, RefGP = import_reference(ref_root)
    c, noise, alpha = 0.1, 1e-4, 1e-10
    seeds = range(8)
    # a committed camera point cloud (D = 3, O = 3): centred, unit scale
    with np.load(os.path.join(HERE, "point_cloud_pan.npz"), allow_pickle=False) as f:
        cloud = np.unique(np.asarray(f["cloud"], np.float64), axis=0)
    cloud = (cloud - cloud.mean(0)) / np.abs(cloud - cloud.mean(0)).max()
    Yc = 0.05 * np.sin(4 * cloud)
    Xq = cloud[np.random.default_rng(7).choice(len(cloud), 100, replace=False)] + 0.01 * np.random.default_rng(8).standard_normal((100, 3))
    build_case(al, RefGP, "pan_cloud", cloud, Yc, Xq, c, noise, alpha, 0, 80, [np.full(3, l) for l in (0.5, 0.6, 0.7, 0.8, 1.0)], seeds)
    X, Y, Xq = uniform_pool(1500, 2, 2, 1)
    build_case(al, RefGP, "uniform_2d", X, Y, Xq, c, noise, alpha, 0, 200, [np.full(2, l) for l in (0.15, 0.2, 0.25, 0.3)], seeds)
    X, Y, Xq = uniform_pool(1000, 3, 3, 2)
    build_case(al, RefGP, "matern52_3d", X, Y, Xq, c, noise, alpha, 2.5, 100, [np.full(3, l) for l in (0.5, 0.7, 1.0)], seeds)
    X, Y, Xq = uniform_pool(800, 5, 5, 3)
    build_case(al, RefGP, "uniform_5d", X, Y, Xq, c, noise, alpha, 0, 100, [np.array([1.0, 1.2, 0.9, 1.1, 1.3]) * s for s in (1.0, 1.3, 1.6)], seeds)


if __name__ == "__main__":
    main(sys.argv[1])
