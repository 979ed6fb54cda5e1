"""numpy restatement of the device epilogue of the transport (csrc/gpt_transport.hip): the affine part, the push-forward of
positions and velocities, and the quaternion of the rotation closest to the Jacobian.

The quaternion mirrors the device algorithm in float64: the same symmetric 4 x 4 matrix, cyclic Jacobi with the same rotation
formula, pair order and fixed sweep count, the same choice of eigenvector (largest diagonal entry, lowest index on a tie,
normalised, sign w >= 0).  Everything else is np.longdouble: `epilogue` is the exact value of every output given the
posterior arrays it consumed, together with S = the same expression with absolute values on every product, the scale of
the rounding floor of the device's short fp64 sums."""
import numpy as np

SWEEPS = 6                                  # TRANSPORT_JACOBI_SWEEPS of csrc/gpt_transport.h
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
LD = np.longdouble
EPS = np.finfo(np.float64).eps


def bar_itzhack_matrix(M, dtype=np.float64):
    """K(M) of Bar-Itzhack (2000), as quaternion.py builds it: its dominant eigenvector is (x, y, z, w)."""
    M = np.asarray(M, dtype=dtype).reshape(-1, 3, 3)
    K = np.zeros((M.shape[0], 4, 4), dtype=dtype)
    K[:, 0, 0] = M[:, 0, 0] - M[:, 1, 1] - M[:, 2, 2]
    K[:, 1, 1] = M[:, 1, 1] - M[:, 0, 0] - M[:, 2, 2]
    K[:, 2, 2] = M[:, 2, 2] - M[:, 0, 0] - M[:, 1, 1]
    K[:, 3, 3] = M[:, 0, 0] + M[:, 1, 1] + M[:, 2, 2]
    K[:, 0, 1] = K[:, 1, 0] = M[:, 1, 0] + M[:, 0, 1]
    K[:, 0, 2] = K[:, 2, 0] = M[:, 2, 0] + M[:, 0, 2]
    K[:, 1, 2] = K[:, 2, 1] = M[:, 2, 1] + M[:, 1, 2]
    K[:, 0, 3] = K[:, 3, 0] = M[:, 2, 1] - M[:, 1, 2]
    K[:, 1, 3] = K[:, 3, 1] = M[:, 0, 2] - M[:, 2, 0]
    K[:, 2, 3] = K[:, 3, 2] = M[:, 1, 0] - M[:, 0, 1]
    return K / dtype(3)


def _rotate(K, V, p, q):
    apq = K[:, p, q].copy()
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        theta = (K[:, q, q] - K[:, p, p]) / (2.0 * apq)
        t = np.copysign(1.0, theta) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        t = np.where(apq == 0.0, 0.0, t)
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        tau = s / (1.0 + c)
        h = t * apq
        K[:, p, p] -= h
        K[:, q, q] += h
        K[:, p, q] = K[:, q, p] = 0.0
        for r in range(4):
            if r != p and r != q:
                g, f = K[:, r, p].copy(), K[:, r, q].copy()
                K[:, r, p] = K[:, p, r] = g - s * (f + tau * g)
                K[:, r, q] = K[:, q, r] = f + s * (g - tau * f)
            g, f = V[:, r, p].copy(), V[:, r, q].copy()
            V[:, r, p] = g - s * (f + tau * g)
            V[:, r, q] = f + s * (g - tau * f)


def jacobi_dominant(K, sweeps=SWEEPS):
    """(v (n,4) unit, lambda (n,), gap (n,) = (lambda_4 - lambda_3) / |K|_F) of symmetric 4 x 4 matrices, float64, the device's way."""
    K = np.array(K, dtype=np.float64)
    n = K.shape[0]
    fro = np.sqrt(np.sum(K * K, axis=(1, 2)))
    V = np.broadcast_to(np.eye(4), (n, 4, 4)).copy()
    for _ in range(sweeps):
        for p, q in PAIRS:
            _rotate(K, V, p, q)
    diag = K[:, np.arange(4), np.arange(4)]
    with np.errstate(invalid="ignore", divide="ignore"):
        best = np.argmax(np.where(np.isnan(diag), -np.inf, diag), axis=1)       # first maximum: the lowest index on a tie
        v = V[np.arange(n), :, best]
        lam = diag[np.arange(n), best]
        rest = np.sort(diag, axis=1)[:, -2]
        v = v / np.sqrt(np.sum(v * v, axis=1))[:, None]
        return v, lam, (lam - rest) / fro


def quaternion_closest(Jp):
    """(q (n,4) as w,x,y,z with w >= 0, gap (n,)) of the rotation closest to each 3 x 3 matrix."""
    v, _, gap = jacobi_dominant(bar_itzhack_matrix(Jp))
    q = np.stack([v[:, 3], v[:, 0], v[:, 1], v[:, 2]], axis=1)
    q[q[:, 0] < 0] *= -1.0
    return q, gap


def quaternion_multiply(a, b):
    aw, ax, ay, az = np.moveaxis(a, -1, 0)
    bw, bx, by, bz = np.moveaxis(b, -1, 0)
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], axis=-1)


def quaternion_checks(K, v):
    """The four measures of the eigenvector tests, evaluated in longdouble against numpy's eigh, each in units of eps:
    residual |Kv - (v'Kv)v| / |K|_F, eigenvalue (lambda_max - v'Kv) / |K|_F, norm ||v| - 1|, vector min|+-v - u| gap / |K|_F
    (NaN where the gap is below 1e-3 |K|_F), and the share of such cases."""
    Kl, vl = np.asarray(K, dtype=LD), np.asarray(v, dtype=LD)
    fro = np.sqrt(np.sum(Kl * Kl, axis=(1, 2)))
    Kv = np.einsum("nij,nj->ni", Kl, vl)
    ray = np.sum(vl * Kv, axis=1)
    w, U = np.linalg.eigh(np.asarray(K, dtype=np.float64))
    u = U[:, :, -1].astype(LD)
    gap = (w[:, -1] - w[:, -2]).astype(LD)
    wide = gap >= 1e-3 * fro
    dist = np.minimum(np.linalg.norm((vl - u).astype(np.float64), axis=1), np.linalg.norm((vl + u).astype(np.float64), axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        vec = np.where(wide, dist * gap / fro, np.nan)
    return {"residual": np.sqrt(np.sum((Kv - ray[:, None] * vl) ** 2, axis=1)) / fro / EPS, "eigenvalue": (w[:, -1] - ray) / fro / EPS,
            "norm": np.abs(np.sqrt(np.sum(vl * vl, axis=1)) - 1) / EPS, "vector": vec / EPS, "left_out": float(np.mean(~wide)),
            "gap": (gap / fro).astype(np.float64)}


def _det(B):
    D = B.shape[-1]
    if D == 1:
        return B[:, 0, 0], np.abs(B[:, 0, 0])
    if D == 2:
        t = [B[:, 0, 0] * B[:, 1, 1], -B[:, 0, 1] * B[:, 1, 0]]
    else:
        t = [B[:, 0, 0] * B[:, 1, 1] * B[:, 2, 2], -B[:, 0, 0] * B[:, 1, 2] * B[:, 2, 1], -B[:, 0, 1] * B[:, 1, 0] * B[:, 2, 2],
             B[:, 0, 1] * B[:, 1, 2] * B[:, 2, 0], B[:, 0, 2] * B[:, 1, 0] * B[:, 2, 1], -B[:, 0, 2] * B[:, 1, 1] * B[:, 2, 0]]
    return sum(t), sum(np.abs(x) for x in t)


def epilogue(pos, R, scale, c_src, c_dst, R_jac, mean, vel=None, J=None, Jvar=None, J_ori=None):
    """Exact (longdouble) value of every output of the device epilogue from its own inputs, as {name: (value, S)}; S is the
    same expression with absolute values on every product.  J_phi: (I + J_ori) R_jac, whose quaternion the caller takes."""
    pos, R, c_src, c_dst, Rj, mean = (np.asarray(a, dtype=LD) for a in (pos, R, c_src, c_dst, R_jac, mean))
    scale = LD(scale)
    D = pos.shape[1]
    eye = np.eye(D, dtype=LD)
    rot = scale * ((pos - c_src) @ R.T) + c_dst
    rot_S = np.abs(scale) * ((np.abs(pos) + np.abs(c_src)) @ np.abs(R).T) + np.abs(c_dst)
    out = {"pos_rot": (rot, rot_S), "pos_out": (rot + mean, rot_S + np.abs(mean))}
    if J is not None:
        J = np.asarray(J, dtype=LD)
        B = (eye + J) @ Rj
        det, det_S = _det(B)
        _, det_S = _det((eye + np.abs(J)) @ np.abs(Rj))
        out["det_vel"] = (det, det_S)
    if vel is not None:
        vel = np.asarray(vel, dtype=LD)
        vr, vr_S = vel @ Rj.T, np.abs(vel) @ np.abs(Rj).T
        if J is not None:
            out["vel_out"] = (vr + np.einsum("nod,nd->no", J, vr), vr_S + np.einsum("nod,nd->no", np.abs(J), vr_S))
        if Jvar is not None:
            Jvar = np.asarray(Jvar, dtype=LD)
            out["vel_var"] = (np.sum(Jvar * vr ** 2, axis=1), np.sum(np.abs(Jvar) * vr_S ** 2, axis=1))
    if J_ori is not None:
        J_ori = np.asarray(J_ori, dtype=LD)
        Jp = (eye + J_ori) @ Rj
        det, _ = _det(Jp)
        _, det_S = _det((eye + np.abs(J_ori)) @ np.abs(Rj))
        out["det_ori"] = (det, det_S)
        out["J_phi"] = (Jp, (eye + np.abs(J_ori)) @ np.abs(Rj))
    return out


def transport_all(pt, pos, vel=None, ori=None):
    """(positions, std, velocities, velocity variance, orientations) of a fitted PolicyTransportation `pt`, computed the fused
    way: one evaluation of the delta_map's posterior at gamma(pos), one of its Jacobian at pos, then `epilogue`."""
    aff, gp = pt.affine_transform, pt.delta_map
    pos = np.asarray(pos, dtype=np.float64)
    D = pos.shape[1]
    rot = (LD(aff.scale) * ((pos.astype(LD) - aff.S_centroid.astype(LD)) @ aff.rotation_matrix.astype(LD).T)
           + aff.T_centroid.astype(LD)).astype(np.float64)
    mean, std = gp.predict(rot, return_std=True)
    J = Jvar = J_ori = None
    if vel is not None:
        J, Jvar = gp.derivative(rot, return_var=True)
        Jvar = Jvar[:, 0, :]
    if ori is not None:
        J_ori = gp.derivative(pos)
    e = epilogue(pos, aff.rotation_matrix, aff.scale, aff.S_centroid, aff.T_centroid, aff.rotation_matrix, mean, vel, J, Jvar, J_ori)
    f64 = lambda k: e[k][0].astype(np.float64)
    res = [f64("pos_out"), std, None, None, None]
    if vel is not None:
        res[2] = f64("vel_out")
        res[3] = np.repeat(f64("vel_var")[:, None], D, axis=1)
    if ori is not None and D == 3:
        q, _ = quaternion_closest(f64("J_phi"))
        res[4] = quaternion_multiply(q, np.asarray(ori, dtype=np.float64))
    return tuple(res)
