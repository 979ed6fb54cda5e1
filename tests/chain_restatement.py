"""numpy restatement of the transported policy through a chain of transports (csrc/gpt_chain.hip, gpt_pullback_chain of
include/gpt_hip.h):  Phi = Phi_{K-1} o ... o Phi_0,  x = Phi^-1(y),  vel = J_Phi(x) f(x).  Not a test; imported by
tests/test_pullback_chain.py, examples and tools.

`chain` composes tests/pullback_restatement.pullback stage by stage, from the last stage to the first, the x of one stage the y
of the one before; a guess x0 of the source-space preimage is pushed forward through the stages' means first, g_0 = x0,
g_{k+1} = gamma_k(g_k) + mean_k(gamma_k(g_k)), and stage k starts at gamma_k(g_k).  `velocity` and `variances` are the
chained products in np.longdouble AT THE ARRAYS GIVEN (what the device returned), each with S = the same product with absolute
values on every term; a chained product of K + 1 factors is held to 16 (K + 1) eps S, the 16 eps S per product of
tests/test_transport_fused.py once per product."""
import numpy as np

from tests import inverse_map_restatement as INV
from tests import pullback_restatement as P

LD = np.longdouble
EPS = np.finfo(np.float64).eps


def push_guess(models, affs, x0):
    """[g_0, ..., g_{K-1}]: the guess of every stage's source-side preimage, in float64."""
    g, out = np.asarray(x0, dtype=np.float64), []
    for k, (m, aff) in enumerate(zip(models, affs)):
        out.append(g)
        if k + 1 < len(models):
            z0 = P.affine_forward(aff, g)
            g = z0 + m.mean(z0)[0].astype(np.float64)
    return out


def chain(models, dyn_model, affs, y, x0=None, rtol=1e-10, max_passes=64):
    """The call in float64 over the restated iteration: x, f, vel (M,D), status (M,) and the stage-major stage_x, stage_z,
    stage_A, stage_status, stage_passes, stage_residual, stage_det."""
    K = len(models)
    guesses = [None] * K if x0 is None else push_guess(models, affs, x0)
    yk = np.asarray(y, dtype=np.float64)
    per = [None] * K
    for k in range(K - 1, -1, -1):
        per[k] = P.pullback(models[k], dyn_model, affs[k], yk, x0=guesses[k], rtol=rtol, max_passes=max_passes)
        yk = per[k]["x"]
    out = {"stage_" + name: np.stack([per[k][key] for k in range(K)])
           for name, key in (("x", "x"), ("z", "z"), ("A", "A"), ("status", "status"), ("passes", "passes"), ("residual", "residual"),
                             ("det", "det"))}
    out["x"] = per[0]["x"]
    status = np.full(len(yk), INV.CONVERGED, dtype=per[0]["status"].dtype)
    for k in range(K - 1, -1, -1):                     # the first stage in solve order that is not CONVERGED
        status = np.where(status == INV.CONVERGED, per[k]["status"], status)
    out["status"] = status
    f = dyn_model.mean(out["x"])[0]
    v = f
    for k in range(K):
        A = np.eye(yk.shape[1], dtype=LD)[None] + models[k].jac(per[k]["z"])[0]
        Rj = np.asarray(affs[k].get("R_jac", affs[k]["R"]), dtype=LD)
        v = np.einsum("mod,md->mo", A @ Rj, v)
    out["f"], out["vel"] = f.astype(np.float64), v.astype(np.float64)
    return out


def first_failing(stage_status):
    """status (M,) from stage_status (K,M): the code of the first stage in solve order (K-1 first) that is not CONVERGED."""
    status = np.full(stage_status.shape[1], INV.CONVERGED, dtype=stage_status.dtype)
    for k in range(stage_status.shape[0] - 1, -1, -1):
        status = np.where(status == INV.CONVERGED, stage_status[k], status)
    return status


def _stage_B(affs, stage_A):
    """[(B_k, |B_k| formed from absolute values)] with B_k = A_k R_jac,k in longdouble."""
    out = []
    for aff, A in zip(affs, np.asarray(stage_A, dtype=LD)):
        Rj = np.asarray(aff.get("R_jac", aff["R"]), dtype=LD)
        out.append((A @ Rj, np.abs(A) @ np.abs(Rj)))
    return out


def velocity(affs, f, stage_A):
    """(B_{K-1} ... B_0 f, 16 (K + 1) eps S) in longdouble at the f and A_k given."""
    v = np.asarray(f, dtype=LD)
    S = np.abs(v)
    for B, BS in _stage_B(affs, stage_A):
        v, S = np.einsum("mod,md->mo", B, v), np.einsum("mod,md->mo", BS, S)
    return v, 16 * (len(affs) + 1) * EPS * S


def variances(affs, f, stage_A, var_dyn, stage_Jvar, std_offset):
    """{vel_var_dyn, vel_var_map: (exact value (M,D), 16 (K + 1) eps S)} in longdouble at the arrays given:
    vel_var_dyn[m,i] = s^2 sum_j P[i,j]^2, s = sqrt(var_dyn) - std_offset, P = B_{K-1} ... B_0;
    vel_var_map[m,i] = sum_k sigma_k^2 sum_j (B_{K-1} ... B_{k+1})[i,j]^2, sigma_k^2 = sum_d Jvar_k[d] (R_jac,k v_{k-1})_d^2,
    v_{-1} = f, v_k = B_k v_{k-1}."""
    K = len(affs)
    Bs = _stage_B(affs, stage_A)
    f = np.asarray(f, dtype=LD)
    M, D = f.shape
    eye = np.broadcast_to(np.eye(D, dtype=LD), (M, D, D))
    tails = [None] * K                                     # (P_{>k}, the same from absolute values)
    Q, QS = eye, eye
    for k in range(K - 1, -1, -1):
        tails[k] = (Q, QS)
        Q, QS = Q @ Bs[k][0], QS @ Bs[k][1]
    out = {}
    if var_dyn is not None:
        sd = np.sqrt(np.asarray(var_dyn, dtype=LD))
        out["vel_var_dyn"] = (((sd - LD(std_offset)) ** 2)[:, None] * np.sum(Q ** 2, axis=2),
                              16 * (K + 1) * EPS * ((sd + abs(LD(std_offset))) ** 2)[:, None] * np.sum(QS ** 2, axis=2))
    if stage_Jvar is not None:
        v, vS = f, np.abs(f)
        total, total_S = np.zeros((M, D), dtype=LD), np.zeros((M, D), dtype=LD)
        for k in range(K):
            Rj = np.asarray(affs[k].get("R_jac", affs[k]["R"]), dtype=LD)
            Jvar = np.asarray(stage_Jvar[k], dtype=LD)
            g, gS = v @ Rj.T, vS @ np.abs(Rj).T
            sig, sig_S = np.sum(Jvar * g ** 2, axis=1), np.sum(np.abs(Jvar) * gS ** 2, axis=1)
            total = total + sig[:, None] * np.sum(tails[k][0] ** 2, axis=2)
            total_S = total_S + sig_S[:, None] * np.sum(tails[k][1] ** 2, axis=2)
            v, vS = np.einsum("mod,md->mo", Bs[k][0], v), np.einsum("mod,md->mo", Bs[k][1], vS)
        out["vel_var_map"] = (total, 16 * (K + 1) * EPS * total_S)
    return out


def carried_bound(models, affs, stage_z, stage_y, rtol):
    """The distance a CONVERGED chain may keep from the exact preimage, to first order.  Stage k solves z + psi_k(z) = y_k for a
    y_k that is off by e_{k+1}, what the stages solved before it left, plus the float64 rounding of y_k itself, 8 eps (1 + |y_k|)
    (tests/test_pullback_policy.py): that moves z by |A_k^-1|_2 times as much; its own iteration adds
    inverse_map_restatement.error_bound (twice, as the tests of the single map allow); the affine inverse divides by scale_k and
    rounds, 64 eps |x_k|.  stage_y[k]: the y stage k solved for.  Returns e_0 (M,)."""
    err = 0.0
    for k in range(len(models) - 1, -1, -1):
        bound, _ = INV.error_bound(models[k], stage_z[k], stage_y[k], rtol)
        _, A = INV.residual_and_jacobian(models[k], stage_z[k], stage_y[k])
        inv_norm = 1.0 / np.linalg.svd(A, compute_uv=False)[:, -1]
        x = P.affine_inverse(affs[k], stage_z[k])[0].astype(np.float64)
        err = (2 * bound + inv_norm * (err + 8 * EPS * (1 + np.linalg.norm(stage_y[k], axis=1)))) / affs[k]["scale"] + \
            64 * EPS * np.linalg.norm(x, axis=1)
    return err
