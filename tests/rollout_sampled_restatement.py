"""numpy restatement of the sampled rollout (csrc/gpt_rollout_sampled.h, gpt_rollout_sampled of include/gpt_hip.h), in fp64 and in
np.longdouble.  Not a test; imported by tests/test_rollout_sampled_cpu.py, tests/test_rollout_sampled.py, examples and tools.

One path of ONE function drawn from the posterior of a dynamics GP (no maps here: x_t = y_t), z the caller's standard normals:
    f_t    = the mean at x_t
    u_t    = W k*(x_t),  pvar_t = (c + nugget) - u_t . u_t
    c_ts   = k(x_t, x_s) - u_t . u_s                                  s < t, k the kernel without noise
    g_ts   = (c_ts - sum_{r<s} g_tr g_sr) / g_ss, s ascending         row t of the lower factor G
    cvar_t = pvar_t - sum_{s<t} g_ts^2, s ascending
    cvar_t NaN or <= FLOOR_ULPS_TOTAL 2^-52 (c + nugget): the path ends at step t, status DEGENERATE; else g_tt = sqrt(cvar_t)
    fs_t   = f_t + sum_{r<=t} g_tr z_r, r ascending from 0
    y_t+1  = y_t + dt fs_t
End rule and NaN filling are tests/rollout_restatement.rollout's: a path ends where its next point is not finite; the step's x and
f (and, unless degenerate, vel) are recorded, every later row is NaN.

`Model` holds the fitted dynamics in the precision asked for: in fp64 the library's algebra (tests/posterior_restatement's
posterior_float64: sources stored as X / l, coordinates carrying 1 / sqrt2, k* = pre exp(ln c - t), explicit W = L^-1 from LAPACK),
in longdouble plain formulas with the column-loop Cholesky.  `path_terms` evaluates the definition at GIVEN points, which is what
the step-local checks need: the dynamics amplifies rounding, so two rollouts are compared at the same points, never end to end."""
import numpy as np

from tests import posterior_restatement as PR

LD = np.longdouble
EPS = 2.0 ** -52
CONVERGED, DEGENERATE = 0, 4
FLOOR_ULPS_TOTAL = PR.MARGIN * PR.FLOOR_ULPS          # 1024: the bound the project holds variances to


def floor(c, nugget):
    return FLOOR_ULPS_TOTAL * EPS * (c + nugget)


class Model:
    def __init__(self, X, Y, c, ls, noise, jitter, kind, ty=np.float64):
        X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
        self.ty, self.kind, self.N, self.D = ty, kind, X.shape[0], X.shape[1]
        self.c, self.noise = ty(c), ty(noise)
        lsv = PR._full_ls(ls, self.D)
        if ty is np.float64:
            self.inv = 1.0 / lsv
            self.Xs = X * self.inv
            k = PR.shapes(PR._sq(self.Xs, self.Xs)[0], kind, ty)[0]
            K = c * k
            K[np.diag_indices_from(K)] += noise + jitter
            self.W = np.linalg.inv(np.linalg.cholesky(K))
            self.alpha = self.W.T @ (self.W @ Y)
        else:
            self.inv = ty(1) / lsv.astype(ty)
            self.Xs = X.astype(ty) * self.inv
            k = PR.shapes(PR._sq(self.Xs, self.Xs)[0], kind, ty)[0]
            K = self.c * k
            K[np.diag_indices_from(K)] += self.noise + ty(jitter)
            L = PR.cholesky_columns(K)
            self.W = PR.forward_substitution(L, np.eye(self.N, dtype=ty))
            self.alpha = PR.backward_substitution(L, PR.forward_substitution(L, Y.astype(ty)))

    def _cross(self, A, Bs):
        """c k between the points A (m,D) and the scaled points Bs (n,D) = B / l."""
        A = np.asarray(A, dtype=self.ty)
        if self.ty is np.float64:
            h = PR._sq(A * (self.inv * PR.RS2), Bs * PR.RS2)[0]
            return PR.shapes(h + h, self.kind, self.ty, lnc=np.log(self.c))[0]
        return self.c * PR.shapes(PR._sq(A * self.inv, Bs)[0], self.kind, self.ty)[0]

    def kstar(self, x):
        return self._cross(x, self.Xs)                           # (m, N)

    def prior(self, xa, xb):
        return self._cross(xa, np.asarray(xb, dtype=self.ty) * self.inv)

    def mean(self, x):
        """(mean (m,O),): row by row, so that a point's mean does not depend on the batch it is evaluated in."""
        ks = self.kstar(x)
        return (np.stack([k @ self.alpha for k in ks]),)


def factor_row(model, xt, Xprev, Uprev, G, nugget):
    """Row t of the definition at the point xt (D,), given the t earlier points, their u (t,N) and the factor so far (t,t).
    Returns (u_t, pvar_t, g_t (t,), cvar_t)."""
    ty = model.ty
    u = model.W @ model.kstar(xt[None])[0]
    pvar = (model.c + ty(nugget)) - u @ u
    t = len(Xprev)
    g = np.zeros(t, dtype=ty)
    if t:
        cts = model.prior(xt[None], Xprev)[0] - Uprev @ u
        for s in range(t):
            g[s] = (cts[s] - G[s, :s] @ g[:s]) / G[s, s]
    dsum = ty(0)
    for s in range(t):
        dsum = dsum + g[s] * g[s]
    return u, pvar, g, pvar - dsum


def path_terms(model, xs, nugget):
    """The definition at the given points xs (T,D) of one path: {f (T,O), pvar (T,), cvar (T,), chol (T,T), cov (T,T)}; cov is the
    path's posterior covariance with the nugget on its diagonal, k(x_t, x_s) - u_t . u_s, which chol factors.  A degenerate pivot
    leaves NaN from its row on."""
    ty = model.ty
    xs = np.asarray(xs, dtype=ty)
    T = len(xs)
    f = model.mean(xs)[0]
    U = np.zeros((T, model.N), dtype=ty)
    G = np.full((T, T), np.nan, dtype=ty)
    pvar, cvar = np.full(T, np.nan, dtype=ty), np.full(T, np.nan, dtype=ty)
    for t in range(T):
        U[t], pvar[t], g, cvar[t] = factor_row(model, xs[t], xs[:t], U[:t], G[:t, :t], nugget)
        if not cvar[t] > floor(model.c, ty(nugget)):
            break
        G[t, :t], G[t, t], G[t, t + 1:] = g, np.sqrt(cvar[t]), 0
    cov = model.prior(xs, xs) - U @ U.T
    cov[np.diag_indices_from(cov)] = (model.c + ty(nugget)) - np.einsum("tn,tn->t", U, U)
    return {"f": f, "pvar": pvar, "cvar": cvar, "chol": G, "cov": cov}


def draw(f, g_row, z):
    """fs = f + sum_r g_r z_r, r ascending from 0, each product and sum rounded on its own."""
    acc = np.zeros_like(f)
    for r in range(len(g_row)):
        acc = acc + g_row[r] * z[r]
    return f + acc


def rollout(model, y0, normals, n_steps, nugget, dt=1.0):
    """{path (P,T+1,D), vel, x, f (P,T,D), pvar, cvar (P,T), chol (P,T,T), steps_done, status (P,)} of the definition, in the
    model's precision.  normals (P,T,D)."""
    ty = model.ty
    y0 = np.asarray(y0, dtype=ty)
    P, D = y0.shape
    T = int(n_steps)
    normals = np.asarray(normals, dtype=ty).reshape(P, T, D)
    nan = lambda *s: np.full(s, np.nan, dtype=ty)
    out = {"path": nan(P, T + 1, D), "vel": nan(P, T, D), "x": nan(P, T, D), "f": nan(P, T, D), "pvar": nan(P, T), "cvar": nan(P, T),
           "chol": nan(P, T, T), "steps_done": np.zeros(P, dtype=np.int32), "status": np.full(P, CONVERGED, dtype=np.int32)}
    out["path"][:, 0] = y0
    fl = floor(model.c, ty(nugget))
    for p in range(P):
        U = np.zeros((T, model.N), dtype=ty)
        G = out["chol"][p]
        for t in range(T):
            x = out["path"][p, t].copy()
            out["x"][p, t] = x
            out["f"][p, t] = f = model.mean(x[None])[0][0]
            U[t], out["pvar"][p, t], g, cvar = factor_row(model, x, out["x"][p, :t], U[:t], G[:t, :t], nugget)
            out["cvar"][p, t] = cvar
            if not cvar > fl:
                out["status"][p] = DEGENERATE
                break
            G[t, :t], G[t, t], G[t, t + 1:] = g, np.sqrt(cvar), 0
            out["vel"][p, t] = fs = draw(f, G[t, :t + 1], normals[p])
            with np.errstate(over="ignore", invalid="ignore"):
                nxt = x + ty(dt) * fs
            if not np.all(np.isfinite(nxt)):
                break
            out["path"][p, t + 1] = nxt
            out["steps_done"][p] = t + 1
    return out
