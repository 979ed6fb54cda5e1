"""Headless fold-free transport of the 2-D letter-S: the reference's
example/2D/surface_generalization_with_diffeomorphism_optimization.py with GaussianProcessTransportationDiffeo.

The unconstrained fit of the letter-S transport folds (det(I + J_psi) <= 0 at 21 of the 400 demonstration points), so the
transported policy has no single preimage there and a rollout through it ends early.  The reference searches the upper bound of
the RBF length-scale with optuna and scores each trial by the error of an inverse surrogate GP; here the trials are a grid, all of
them are fitted by one device search and scored by one device scan, and the criterion is the sign of det(I + J_psi) itself:

    python examples/diffeomorphic_letter_s_2d.py

prints the trial table, what either criterion picks, and the rollout of the demonstration's own dynamics from the moved
demonstration's start (1000 steps of dt = 1) through the unconstrained map and through the fold-free one.
Data: tests/golden/letterS_2d.npz."""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sklearn.gaussian_process.kernels import RBF, WhiteKernel, ConstantKernel as C  # noqa: E402

from gaussian_process_transportation_amd import GaussianProcess, GaussianProcessTransportationDiffeo  # noqa: E402


def fit(g, **kw):
    t = GaussianProcessTransportationDiffeo(verbose=False)
    t.source_distribution, t.target_distribution, t.training_traj = g["source"], g["target"], g["demo"]
    np.random.seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t.optimize_diffeomorphism(**kw)
    return t


def main(verbose=True, n_trials=10, n_steps=1000):
    g = np.load(os.path.join(ROOT, "tests", "golden", "letterS_2d.npz"))
    dynamics = GaussianProcess(kernel=C(0.3) * RBF([1.5, 2.5]) + WhiteKernel(0.01), optimizer=None, verbose=False).fit(g["demo"], g["delta"])
    out = {}
    fits = (("unconstrained", dict(max_lengthscales=[20.0])), ("error", dict(n_trials=n_trials, criterion="error")),
            ("fold_free", dict(n_trials=n_trials, criterion="fold_free")))
    for name, kw in fits:
        t = fit(g, **kw)
        moved = t.method.transport(g["demo"], return_std=False)[0]
        error = t.check_invertibility()
        path, info = t.rollout_policy(dynamics, moved[:1], n_steps, dt=1.0, x0=g["demo"][:1], return_info=True)
        out[name] = dict(transport=t, moved=moved, error=error, path=path, steps_done=int(info["steps_done"][0]))
    if verbose:
        tr = out["fold_free"]["transport"].diffeo_trials_
        print(f"{n_trials} trials, one device search ({6 * n_trials} runs) and one device scan; the evaluation set is the affine-moved demonstration (400 points)")
        print(" max_lengthscale   fitted length-scale         LML   surrogate error   min det(I+J)   folds at")
        for k in range(n_trials):
            ls = np.exp(tr["theta"][k][1:3])
            print(f"   {tr['max_lengthscale'][k]:8.2f}      {ls[0]:7.2f} {ls[1]:7.2f}    {tr['lml'][k]:9.2f}    {tr['error'][k]:10.1f}     {tr['min_det'][k]:+9.3f}    {int(tr['n_fold'][k]):4d}")
        for name, _ in fits:
            o = out[name]
            t = o["transport"]
            print(f"{name:>13}: max_lengthscale {t.max_lengthscale_:5.2f}, folds at {t.n_fold_:2d} of 400 points (min det {t.min_det_:+.3f}), surrogate error "
                  f"{o['error']:6.1f}; rollout from the demonstration's start: {o['steps_done']} of {n_steps} steps done")
    return out


if __name__ == "__main__":
    main()
