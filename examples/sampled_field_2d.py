"""Headless, seeded: ONE plausible policy as a whole vector field, and where the same plausible policies take the robot from many
starts.  The scene is examples/obstacle_chain_2d.py's two-stage chain on the letter-S (tests/golden/letterS_2d.npz): the
demonstration moved to the new surface, then bent round an obstacle; the dynamics GP is fitted to the demonstration's steps.

GaussianProcess.sample_functions draws 8 whole functions from the posterior of the dynamics by pathwise conditioning (random
Fourier features for the prior, one solve against the data per function).  Unlike the paths of rollout_samples, each of which
is a function of its own known only along itself, a drawn function exists everywhere: it is evaluated on a 100 x 100 grid (the
sampled field a stream plot would show), and rolled out for 1000 steps, the reference's plot_traj_evolution, through both maps from
the demonstration's start and from a 10 x 10 grid of starts, all starts under the same 8 functions, in one device call
(TransportChain.rollout_functions).  Printed: after 10, 50, 100 and 1000 steps, how many of the 8 paths from the start of the demonstration are alive, their rms
distance from the mean path (while that exists: the first map folds, and a path that reaches the fold ends) and from their own
centre, next to rollout_samples' numbers for the steps that call admits.

--host also runs the numpy loop of the same functions (one transported_policy call per step for the inverse and the per-stage
Jacobians, the functions and the push in numpy).

    python examples/sampled_field_2d.py [--functions 8] [--frequencies 2048] [--steps 1000] [--seed 0] [--host]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sklearn.gaussian_process.kernels import RBF, WhiteKernel, ConstantKernel as C  # noqa: E402

from gaussian_process_transportation_amd import GaussianProcess, GaussianProcessTransportation as Transport, TransportChain, _lib  # noqa: E402
from examples.policy_rollout_2d import rings  # noqa: E402


def kernel_rbf(A, B, c, ls):
    d = (A[:, None, :] - B[None, :, :]) / ls
    return c * np.exp(-0.5 * np.sum(d * d, axis=-1))


def host_loop(chain, dyn, fn, starts, x0, steps, dt=1.0):
    """The loop the device call replaces: every path of a step at once.  Path index = start * S + function."""
    S = len(fn)
    func = np.tile(np.arange(S), len(starts))
    V, amp = fn.weights[func], fn.amplitudes[func]
    R = [np.asarray(m.affine_transform.rotation_matrix) for m in chain.methods]
    path = np.full((len(func), steps + 1, starts.shape[1]), np.nan)
    path[:, 0] = np.repeat(starts, S, axis=0)
    alive, guess = np.arange(len(func)), np.repeat(x0, S, axis=0)
    for t in range(steps):
        if len(alive) == 0:
            break
        _, info = chain.transported_policy(dyn, np.ascontiguousarray(path[alive, t]), x0=guess, return_info=True)
        x, theta = info["x"], info["x"] @ fn.omega.T
        v = (np.einsum("pn,pnd->pd", kernel_rbf(x, dyn.X, dyn._c, dyn._ls), V[alive]) + np.einsum("pj,pjd->pd", np.cos(theta), amp[alive, :, 0])
             + np.einsum("pj,pjd->pd", np.sin(theta), amp[alive, :, 1]))
        for k in range(len(R)):
            v = np.einsum("mij,mj->mi", info["stage_A"][k], v @ R[k].T)
        nxt = path[alive, t] + dt * v
        go = (info["status"] == 0) & np.all(np.isfinite(nxt), axis=1)
        path[alive[go], t + 1] = nxt[go]
        alive, guess = alive[go], np.ascontiguousarray(x[go])
    return path.reshape(len(starts), S, steps + 1, -1)


def main(functions=8, frequencies=2048, steps=1000, seed=0, verbose=True, host=False, n_grid=10, n_field=100):
    g = np.load(os.path.join(ROOT, "tests", "golden", "letterS_2d.npz"))
    dyn = GaussianProcess(kernel=C(0.3) * RBF([1.5, 2.5]) + WhiteKernel(0.01), optimizer=None, verbose=False).fit(g["demo"], g["delta"])
    first = Transport(kernel_transport=C(float(g["constant_value"])) * RBF(g["length_scale"].tolist()) + WhiteKernel(float(g["noise_level"])),
                      optimizer=None, verbose=False)
    first.source_distribution, first.target_distribution = g["source"], g["target"]
    first.fit_transportation()
    moved = first.method.transport(g["demo"], return_std=False)[0]
    second = Transport(kernel_transport=C(4.0) * RBF([6.0, 6.0]) + WhiteKernel(1e-3), optimizer=None, verbose=False)
    second.source_distribution, second.target_distribution = rings(moved[200])
    second.fit_transportation()
    chain = TransportChain([first, second], verbose=False)
    demo = np.ascontiguousarray(g["demo"])
    twice = chain.transport(demo)[0]

    t0 = time.perf_counter()
    fn = dyn.sample_functions(n_functions=functions, n_frequencies=frequencies, random_state=seed)
    t_draw = time.perf_counter() - t0
    # one sampled field: function 0 on a grid over the demonstration, in source space (the stream plot of one plausible policy)
    lo, hi = demo.min(axis=0) - 2, demo.max(axis=0) + 2
    gx, gy = np.meshgrid(np.linspace(lo[0], hi[0], n_field), np.linspace(lo[1], hi[1], n_field))
    grid = np.ascontiguousarray(np.column_stack([gx.ravel(), gy.ravel()]))
    t0 = time.perf_counter()
    field = fn.subset([0]).predict(grid)[0]
    t_field = time.perf_counter() - t0
    mean_field = dyn.predict(grid)
    # the same functions from the start of the demonstration and from a grid of starts, through both maps
    lo, hi = twice.min(axis=0), twice.max(axis=0)
    sx, sy = np.meshgrid(np.linspace(lo[0], hi[0], n_grid), np.linspace(lo[1], hi[1], n_grid))
    starts = np.ascontiguousarray(np.vstack([twice[:1], np.column_stack([sx.ravel(), sy.ravel()])]))
    guesses = chain.inverse_transport(starts, x0=np.ascontiguousarray(np.vstack([demo[:1], np.repeat(demo[200:201], n_grid * n_grid, axis=0)])))
    t0 = time.perf_counter()
    paths, info = chain.rollout_functions(fn, starts, steps, x0=guesses, return_info=True)
    t_roll = time.perf_counter() - t0
    mean_path = chain.rollout(dyn, starts[:1], steps, x0=guesses[:1])[0]

    mean_done = int(chain.rollout(dyn, starts[:1], steps, x0=guesses[:1], return_info=True)[1]["steps_done"][0])

    def spread(p):
        """Per step, over the paths alive there: (how many, their rms distance from the mean path, where it exists; from their own
        centre)."""
        alive = np.all(np.isfinite(p), axis=-1)                                                   # (paths, steps + 1)
        n = alive.sum(axis=0)
        d_mean = np.where(alive, np.sum((np.nan_to_num(p) - np.nan_to_num(mean_path[None, :p.shape[1]])) ** 2, axis=-1), 0.0)
        centre = np.where(alive[..., None], np.nan_to_num(p), 0.0).sum(axis=0) / np.maximum(n, 1)[:, None]
        d_own = np.where(alive, np.sum((np.nan_to_num(p) - centre[None]) ** 2, axis=-1), 0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            to_mean = np.where((n > 0) & (np.arange(p.shape[1]) <= mean_done), np.sqrt(d_mean.sum(axis=0) / n), np.nan)
            to_own = np.where(n > 0, np.sqrt(d_own.sum(axis=0) / n), np.nan)
        return n, to_mean, to_own
    sp = spread(paths[0])
    t_exact = min(steps, _lib.ROLLOUT_SAMPLED_MAX_T)
    exact = chain.rollout_samples(dyn, starts[:1], t_exact, n_samples=functions, nugget=1e-8, random_state=seed, x0=guesses[:1])[0]
    sp_exact = spread(exact)
    out = dict(functions=fn, field=field.reshape(n_field, n_field, 2), grid=grid, paths=paths, info=info, mean_path=mean_path, mean_done=mean_done,
               spread=sp, spread_exact=sp_exact, seconds=t_roll)
    if verbose:
        done = info["steps_done"]
        print(f"dynamics GP kernel: {dyn.kernel}")
        print(f"{functions} functions of {frequencies} frequencies drawn in {t_draw:.3f} s (one solve against the {len(demo)} points each)")
        print(f"function 0 on the {n_field} x {n_field} grid in {t_field:.3f} s: rms distance from the mean field "
              f"{np.sqrt(np.mean(np.sum((field - mean_field) ** 2, axis=-1))):.4f} (rms length of the mean field {np.sqrt(np.mean(np.sum(mean_field ** 2, axis=-1))):.4f})")
        print(f"{len(starts)} starts x {functions} functions = {done.size} paths of {steps} steps through both maps in {t_roll:.3f} s; complete: "
              f"{int(np.sum(done == steps))}; last status: " + ", ".join(f"{n} {int(np.sum(info['status'] == c))}" for c, n in enumerate(_lib.INV_STATUS_NAMES)))
        print(f"the mean path from the demonstration's start ends at step {mean_done} of {steps}" + (" (where the letter-S map folds)" if mean_done < steps else ""))
        print("step   paths alive   rms distance from the mean path   from their own centre   (rollout_samples, latent function: alive, mean path, own centre)")
        fmt = lambda v: "   ended" if np.isnan(v) else f"{v:8.4f}"
        for t in (10, 50, 100, 1000):
            if t <= steps:
                beside = (f"({sp_exact[0][t]}, {fmt(sp_exact[1][t])}, {fmt(sp_exact[2][t])})" if t <= t_exact
                          else f"(not admitted: at most {_lib.ROLLOUT_SAMPLED_MAX_T} steps)")
                print(f"{t:5d}   {sp[0][t]:5d}   {fmt(sp[1][t])}   {fmt(sp[2][t])}   {beside}")
    if host:
        t0 = time.perf_counter()
        host_paths = host_loop(chain, dyn, fn, starts, guesses, steps)
        t1 = time.perf_counter()
        both = np.isfinite(host_paths) & np.isfinite(paths)
        out.update(paths_host=host_paths, seconds_host=t1 - t0)
        if verbose:
            print(f"the same functions in a numpy loop, one transported_policy call per step: {t1 - t0:.3f} s; largest gap between the two sets of "
                  f"paths over their common steps {np.max(np.abs(host_paths - paths)[both]):.3e} (the dynamics amplifies rounding)")
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--functions", type=int, default=8)
    ap.add_argument("--frequencies", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--host", action="store_true", help="also run the numpy loop of the same functions")
    a = ap.parse_args()
    main(a.functions, a.frequencies, a.steps, a.seed, host=a.host)
