"""numpy restatement of the transported policy at target-space points (csrc/gpt_pullback.hip, gpt_pullback_policy of
include/gpt_hip.h):  x = Phi^-1(y),  vel = J_Phi(x) f(x),  Phi = gamma + psi o gamma.  Not a test; imported by
tests/test_pullback_policy.py, examples and tools.

`KernelModel` is a posterior mean c k(., X) alpha of any of the four kernels with its Jacobian, in np.longdouble, together with
S = the same sums with absolute values on every term (the scale of the rounding floor of the device's wave-strided sums); in
float64 it is also a model for tests/inverse_map_restatement.py (mean_jac, abs_sum).  With device_operands=True the model is the
one the device HOLDS: its sources are the stored float64 rows X * (1 / l) (k_scale_x), its query the float64 product
z * ((1 / l) / sqrt 2) and its derivative scale the float64 (1 / l) sqrt 2, so that the distances are formed from the same
operands as on the device and only the arithmetic after them differs.  Where |X / l| is large (the dynamics on the letter-S:
up to 22) the rounding of those operands, a backward error of one eps in X and l, moves a term by more than the floor of the
sums allows for; it belongs to the model, not to the sum.  `pullback` is the whole call over the
restated Newton iteration.  `exact_at` evaluates every output of the device in longdouble AT THE z AND x THE DEVICE RETURNED — the
values its later phases used — so that Newton's path does not enter the comparison."""
import numpy as np

from tests import inverse_map_restatement as INV
from tests.transport_fused_restatement import _det

LD = np.longdouble
EPS = np.finfo(np.float64).eps
SQ3, SQ5 = np.sqrt(LD(3)), np.sqrt(LD(5))
RS2, SQ2 = np.float64(0.70710678118654752440), np.float64(1.41421356237309504880)     # the constants of csrc/gpt_newton.h


class KernelModel:
    """mean(x) = sum_n c k(x, X_n) alpha_n.  nu: None (RBF), 0.5, 1.5 or 2.5."""

    def __init__(self, X, alpha, c, ls, nu=None, device_operands=False):
        self.device_operands = device_operands
        self.X64 = np.asarray(X, dtype=np.float64)
        self.X = np.asarray(X, dtype=LD)
        self.alpha = np.asarray(alpha, dtype=LD).reshape(len(self.X), -1)
        self.c = LD(c)
        self.ls = np.broadcast_to(np.atleast_1d(np.asarray(ls, dtype=LD)), (self.X.shape[1],))
        self.nu = nu

    def _k_g_u(self, z):
        """c k (M,N), c g (M,N) — d k / d z_d = c g u_d — and u (M,N,D) = (X - z) / l^2."""
        if self.device_operands:
            inv = 1.0 / self.ls.astype(np.float64)                                  # fill_params: inv_ls
            Xs = (self.X64 * inv).astype(LD)                                        # k_scale_x
            q = (np.asarray(z, dtype=np.float64) * (inv * RS2)).astype(LD)          # q[d] = z[d] * qsc[d]
            df = Xs[None] * LD(RS2) - q[:, None]                                    # (X - z) / (l sqrt 2)
            r = np.sqrt(2 * np.sum(df * df, axis=-1))
            u = df * (inv * SQ2).astype(LD)                                         # acc * jsc[d]
        else:
            z = np.asarray(z, dtype=LD)
            diff = self.X[None] - z[:, None]
            r = np.sqrt(np.sum((diff / self.ls) ** 2, axis=-1))
            u = diff / self.ls ** 2
        if self.nu is None:
            k = np.exp(-r * r / 2)
            g = k
        elif self.nu == 0.5:
            k, g = np.exp(-r), None
        elif self.nu == 1.5:
            e = np.exp(-SQ3 * r)
            k, g = (1 + SQ3 * r) * e, 3 * e
        elif self.nu == 2.5:
            e = np.exp(-SQ5 * r)
            k, g = (1 + SQ5 * r + 5 * r * r / 3) * e, LD(5) / 3 * (1 + SQ5 * r) * e
        else:
            raise ValueError(self.nu)
        return self.c * k, None if g is None else self.c * g, u

    def mean(self, x):
        """(mean (M,O), S (M,O)) in longdouble."""
        k, _, _ = self._k_g_u(x)
        return k @ self.alpha, np.abs(k) @ np.abs(self.alpha)

    def jac(self, z):
        """(J (M,O,D), S (M,O,D)) in longdouble."""
        _, g, u = self._k_g_u(z)
        gu = g[:, :, None] * u
        return np.einsum("mnd,no->mod", gu, self.alpha), np.einsum("mnd,no->mod", np.abs(gu), np.abs(self.alpha))

    # the protocol of tests/inverse_map_restatement.py, float64
    def mean_jac(self, z):
        return self.mean(z)[0].astype(np.float64), self.jac(z)[0].astype(np.float64)

    def abs_sum(self, z):
        return self.mean(z)[1].astype(np.float64)


def oracle_model(gp):
    """KernelModel of a fitted oracle.gp_oracle.GaussianProcessOracle (RBF)."""
    return KernelModel(gp.X, gp.alpha_, gp.constant_value, gp._ls())


def affine_inverse(aff, z):
    """((z - c_dst) R / scale + c_src, S) in longdouble."""
    R, s = np.asarray(aff["R"], dtype=LD), LD(aff["scale"])
    c_src, c_dst, z = np.asarray(aff["c_src"], dtype=LD), np.asarray(aff["c_dst"], dtype=LD), np.asarray(z, dtype=LD)
    return (z - c_dst) @ R / s + c_src, (np.abs(z) + np.abs(c_dst)) @ np.abs(R) / np.abs(s) + np.abs(c_src)


def affine_forward(aff, x):
    x = np.asarray(x, dtype=np.float64)
    return aff["scale"] * ((x - aff["c_src"]) @ np.asarray(aff["R"]).T) + aff["c_dst"]


def pullback(map_model, dyn_model, aff, y, x0=None, rtol=1e-10, max_passes=64):
    """The call in float64 over the restated iteration: {x, z, f, vel, A, det, residual, passes, status}."""
    y = np.asarray(y, dtype=np.float64)
    z0 = None if x0 is None else affine_forward(aff, x0)
    z, info = INV.inverse_map(map_model, y, z0, rtol=rtol, max_passes=max_passes)
    x = affine_inverse(aff, z)[0].astype(np.float64)
    f = dyn_model.mean(x)[0]
    A = np.eye(y.shape[1], dtype=LD)[None] + map_model.jac(z)[0]
    Rj = np.asarray(aff.get("R_jac", aff["R"]), dtype=LD)
    vel = np.einsum("mod,md->mo", A @ Rj, f)
    return dict(info, x=x, z=z, f=f.astype(np.float64), vel=vel.astype(np.float64), A=A.astype(np.float64))


def exact_at(map_model, dyn_model, aff, y, z, x):
    """{name: (exact value, tolerance)} of x, f, A, vel, det, residual given the z and x the device returned.  Tolerances:
    64 eps S for the wave-strided sums (f, the entries of A); 16 eps S for sums of at most D + 1 products (x, vel), vel with the
    first-order propagation of the floors of f and A through A R_jac f added; det with the floor of A carried through its
    expansion; residual as tests/test_inverse_map.py holds it (both sides carry the rounding of their own sums)."""
    y, z, x = (np.asarray(a, dtype=np.float64) for a in (y, z, x))
    D = y.shape[1]
    Rj = np.asarray(aff.get("R_jac", aff["R"]), dtype=LD)
    out = {}
    xe, xS = affine_inverse(aff, z)
    out["x"] = (xe, 16 * EPS * xS)
    f, fS = dyn_model.mean(x)
    f_floor = 64 * EPS * fS
    out["f"] = (f, f_floor)
    J, JS = map_model.jac(z)
    eye = np.eye(D, dtype=LD)[None]
    A, A_floor = eye + J, 64 * EPS * (eye + JS)
    out["A"] = (A, A_floor)
    g, gS = f @ Rj.T, np.abs(f) @ np.abs(Rj).T
    vel = np.einsum("mod,md->mo", A, g)
    vel_S = np.einsum("mod,md->mo", np.abs(A), gS)
    spread = np.einsum("mod,md->mo", A_floor, np.abs(g)) + np.einsum("mod,md->mo", np.abs(A), f_floor @ np.abs(Rj).T)
    out["vel"] = (vel, 16 * EPS * vel_S + spread)
    det, det_S = _det(A)
    out["det"] = (det, 16 * EPS * det_S + (_det(np.abs(A) + A_floor)[1] - det_S))
    mu, muS = map_model.mean(z)
    out["residual"] = (np.sqrt(np.sum((z.astype(LD) + mu - y.astype(LD)) ** 2, axis=1)),
                       2 * 64 * EPS * np.sqrt(np.sum(muS ** 2, axis=1)) + 8 * EPS * (1 + np.linalg.norm(y, axis=1)))
    return out


def variance_epilogue(aff, f, A, var_dyn, Jvar, std_offset):
    """{vel_var_map, vel_var_dyn: (exact value, 16 eps S)} from the epilogue's own inputs (what the device returned)."""
    Rj = np.asarray(aff.get("R_jac", aff["R"]), dtype=LD)
    f, A = np.asarray(f, dtype=LD), np.asarray(A, dtype=LD)
    g, gS = f @ Rj.T, np.abs(f) @ np.abs(Rj).T
    out = {}
    if Jvar is not None:
        Jvar = np.asarray(Jvar, dtype=LD)
        out["vel_var_map"] = (np.sum(Jvar * g ** 2, axis=1), 16 * EPS * np.sum(np.abs(Jvar) * gS ** 2, axis=1))
    if var_dyn is not None:
        sd = np.sqrt(np.asarray(var_dyn, dtype=LD))
        B, BS = A @ Rj, np.abs(A) @ np.abs(Rj)
        out["vel_var_dyn"] = (((sd - LD(std_offset)) ** 2)[:, None] * np.sum(B ** 2, axis=2),
                              16 * EPS * ((sd + abs(LD(std_offset))) ** 2)[:, None] * np.sum(BS ** 2, axis=2))
    return out
