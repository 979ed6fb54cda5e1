"""numpy restatement of the device hyper-parameter search (bat_optimize, csrc/gpt_batch_opt.hip): the same projected BFGS
iteration, run by run, over the CPU oracle's log_marginal_likelihood.  `batch_optimize_packed` has the signature and the
return value of `_lib.batch_optimize_packed` and stands in for it in the CPU tests.  Not a test module itself.

The iteration, minimising f = -LML over theta = log [c, l.., noise] inside the box lo <= theta <= hi (lo == hi: fixed):
  start   x = clip(x0); f, g there; H = I.  f not finite: NOT_PD_START (lml = -inf).
  step    pg = x - clip(x - g): stop PGTOL if max |pg| <= pgtol; then the caps MAX_ITER, MAX_EVALS.
          active set: fixed components, and those on a bound whose gradient points outward.  d = -H[free, free] g[free], 0 on
          the active set; if d.g >= 0: H = I, d = -g on the free set.
          t = 1 (first iteration: min(1, 1 / |d|)).  Trial xn = clip(x + t d); accepted if f(xn) is finite and
          f(xn) <= f + 1e-4 g.(xn - x); otherwise t /= 2, at most max_ls times, then LINESEARCH (MAX_EVALS if the cap comes first).
          accepted: s = xn - x, y = gn - g (0 on fixed components); BFGS update of H if s.y > 1e-10 |s| |y|;
          stop FTOL if f - fn <= ftol max(|f|, |fn|, 1)."""
import numpy as np

PGTOL, FTOL, MAX_ITER, MAX_EVALS, LINESEARCH, NOT_PD_START = 0, 1, 2, 3, 4, 5
KINDS = ("rbf", "matern12", "matern32", "matern52")
MAX_LS = 30


def search(fun, x0, lo, hi, pgtol=1e-5, ftol=2.22e-9, max_iter=15000, max_evals=15000, max_ls=MAX_LS, trace=None):
    """One run.  fun(x) -> (f, g) with f = +inf where the matrix is not PD.  Returns (x, f, iterations, evaluations, status);
    trace (a list, optional) receives (iteration, halvings, f_trial) of every trial."""
    P = len(lo)
    fixed = lo == hi

    def evaluate(z):
        f, g = fun(z)
        if not (np.isfinite(f) and np.isfinite(g).all()):
            return np.inf, np.zeros(P)
        return float(f), np.asarray(g, dtype=np.float64)

    x = np.clip(np.asarray(x0, dtype=np.float64), lo, hi)
    f, g = evaluate(x)
    evals, it = 1, 0
    if not np.isfinite(f):
        return x, np.inf, 0, 1, NOT_PD_START
    H = np.eye(P)
    while True:
        pg = x - np.clip(x - g, lo, hi)
        if np.max(np.abs(pg)) <= pgtol:
            return x, f, it, evals, PGTOL
        if it >= max_iter:
            return x, f, it, evals, MAX_ITER
        if evals >= max_evals:
            return x, f, it, evals, MAX_EVALS
        active = fixed | ((x <= lo) & (g > 0)) | ((x >= hi) & (g < 0))
        fr = ~active
        d = np.zeros(P)
        d[fr] = -H[np.ix_(fr, fr)] @ g[fr]
        if not d @ g < 0:
            H = np.eye(P)
            d[fr] = -g[fr]
        t = 1.0
        if it == 0:
            t = min(1.0, 1.0 / np.sqrt(d @ d))
        halvings = 0
        while True:
            xn = np.clip(x + t * d, lo, hi)
            fn, gn = evaluate(xn)
            evals += 1
            if trace is not None:
                trace.append((it, halvings, fn))
            if np.isfinite(fn) and fn <= f + 1e-4 * (g @ (xn - x)):
                break
            t *= 0.5
            halvings += 1
            if halvings > max_ls:
                return x, f, it, evals, LINESEARCH
            if evals >= max_evals:
                return x, f, it, evals, MAX_EVALS
        s, y = xn - x, np.where(fixed, 0.0, gn - g)
        sy = s @ y
        if sy > 1e-10 * np.sqrt((s @ s) * (y @ y)):
            rho = 1.0 / sy
            Hy = H @ y
            H = H + ((1.0 + rho * (y @ Hy)) * rho) * np.outer(s, s) - rho * (np.outer(Hy, s) + np.outer(s, Hy))
        f_old = f
        x, f, g = xn, fn, gn
        it += 1
        if f_old - f <= ftol * max(abs(f_old), abs(f), 1.0):
            return x, f, it, evals, FTOL


def launches_of(evaluations, large, evals_per_launch):
    """Launches the relaunch loop makes: per round one for every size class that still has a live run."""
    total = 0
    for cls in (False, True):
        e = evaluations[large == cls]
        if e.size:
            total += int(-(-int(e.max()) // evals_per_launch))
    return total


def batch_optimize_packed(X, Y, n_begin, n_ls, run_model, theta0, bounds, alpha, kernel_type=0, device=0, pgtol=1e-5, ftol=2.22e-9,
                          max_iter=15000, max_evals=15000, evals_per_launch=None):
    """`_lib.batch_optimize_packed` on the CPU oracle: (theta (R, P), lml (R), iterations, evaluations, status, launches)."""
    from oracle import gp_oracle as orc
    run_model = np.asarray(run_model)
    theta0 = np.asarray(theta0, dtype=np.float64)
    bounds = np.asarray(bounds, dtype=np.float64)
    R, P = theta0.shape
    theta, lml = np.empty((R, P)), np.empty(R)
    iters, evals, status = np.zeros(R, dtype=np.int32), np.zeros(R, dtype=np.int32), np.zeros(R, dtype=np.int32)
    for r in range(R):
        b = int(run_model[r])
        Xb, Yb = X[n_begin[b]:n_begin[b + 1]], Y[n_begin[b]:n_begin[b + 1]]

        def fun(z):
            v, g = orc.log_marginal_likelihood(z, Xb, Yb, n_ls, alpha=alpha, kind=KINDS[kernel_type])
            return -v, -g
        x, f, iters[r], evals[r], status[r] = search(fun, theta0[r], bounds[:, 0], bounds[:, 1], pgtol, ftol, max_iter, max_evals)
        theta[r], lml[r] = x, -f
    large = np.diff(n_begin)[run_model] > 32
    return theta, lml, iters, evals, status, launches_of(evals, large, evals_per_launch or 64)


# ------------------------------------------------------------------------------------------------ the comparison's problems
def frame_pair_models(n_pairs=12, n_points=10, seed=0, scale=50.0):
    """Displacement-field models of the multi-frame workload: a 10-point source cloud sent to rotated, shifted, locally bent
    targets, in the pixel-like units the multi-frame kernel's length-scale bounds are meant for (`scale`); X is the source
    after the pair's rigid pre-alignment, Y what the alignment leaves."""
    from gaussian_process_transportation_amd.affine_transform import AffineTransform
    rng = np.random.default_rng(seed)
    source = rng.uniform(-1, 1, (n_points, 2))
    Xs, Ys = [], []
    for _ in range(n_pairs):
        ang = rng.uniform(-0.6, 0.6)
        R = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
        target = source @ R.T + rng.uniform(-0.5, 0.5, 2) + 0.08 * np.sin(3 * source[:, ::-1]) + 0.005 * rng.standard_normal(source.shape)
        aff = AffineTransform(do_scale=False, do_rotation=True, verbose=False)
        aff.fit(source, target)
        X = np.array(aff.predict(source), dtype=np.float64)
        Xs.append(scale * X)
        Ys.append(scale * (target - X))
    return Xs, Ys


def families():
    """[(name, kernel, Xs, Ys)]: tests/test_batch_hyperopt.py's problems under the ARD kernel and under the isotropic kernel
    with fixed noise, and twelve frame-pair models under the multi-frame kernel, whose optimum sits on its bounds."""
    from sklearn.gaussian_process.kernels import RBF, WhiteKernel, ConstantKernel as C
    from tests.test_batch_hyperopt import _kernels, _problems
    Xs, Ys = _problems()
    ard, iso = _kernels()
    multi = C(np.sqrt(10)) * RBF(20, [10, 50]) + WhiteKernel(0.01, [1e-7, 1e-6])
    return [("ard", ard, Xs, Ys), ("iso_fixed_noise", iso, Xs, Ys), ("multi_frame", multi) + frame_pair_models()]


def sklearn_best(kernel, Xs, Ys, restarts=5, seed=5, alpha=1e-10):
    """Per model the LML GaussianProcessRegressor(n_restarts_optimizer=restarts) reaches, fitted in a plain loop from `seed`."""
    import warnings
    from sklearn.gaussian_process import GaussianProcessRegressor
    np.random.seed(seed)
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for X, Y in zip(Xs, Ys):
            out.append(GaussianProcessRegressor(kernel=kernel, alpha=alpha, n_restarts_optimizer=restarts).fit(X, Y).log_marginal_likelihood_value_)
    return np.array(out)
