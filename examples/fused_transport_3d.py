"""The reference's 3-D surface demo with orientations, transported twice on one fitted map: apply_transportation() as the
reference runs it (three posterior calls, the velocity and quaternion algebra in numpy) and with fused=True (one device call:
affine part, posterior, push-forward of velocities and orientations).

    python examples/fused_transport_3d.py

Data: tests/golden/surface_3d.npz (the arrays of the reference's example/3D/data/example.npz) at the hyper-parameters the
reference's optimizer found, and the 102 end-effector quaternions of its robot demo (tests/golden/robot_demo_last.npz), repeated
along the 460-point trajectory."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sklearn.gaussian_process.kernels import RBF, WhiteKernel, ConstantKernel as C  # noqa: E402

from gaussian_process_transportation_amd import GaussianProcessTransportation as Transport  # noqa: E402


def main(verbose=True):
    data = np.load(os.path.join(ROOT, "tests", "golden", "surface_3d.npz"))
    X = data["demo"]
    ori = np.load(os.path.join(ROOT, "tests", "golden", "robot_demo_last.npz"))["training_ori"]
    ori = np.ascontiguousarray(np.resize(ori, (len(X), 4)))
    kernel = C(float(data["constant_value"])) * RBF(length_scale=data["length_scale"].tolist()) + WhiteKernel(float(data["noise_level"]))
    transport = Transport(kernel_transport=kernel, optimizer=None, verbose=False)
    transport.source_distribution = data["source"]
    transport.target_distribution = data["target"]
    transport.fit_transportation()
    out, seconds = {}, {}
    for fused in (False, True, False, True):                       # the first round warms both paths up
        transport.fused = fused
        transport.training_traj, transport.training_delta, transport.training_ori = X, data["delta"], ori
        t0 = time.perf_counter()
        transport.apply_transportation()
        seconds[fused] = time.perf_counter() - t0
        out[fused] = (transport.training_traj, transport.std, transport.training_delta, transport.var_vel_transported, transport.training_ori)
    # what the fused call knows per point and the reference's one-line print does not
    gp, aff = transport.method.delta_map, transport.method.affine_transform
    info = gp.transport_policy(X, aff.rotation_matrix, aff.scale, aff.S_centroid, aff.T_centroid, vel=data["delta"], ori=ori)
    if verbose:
        print(f"apply_transportation(), {len(X)} points, N = {len(data['source'])}: unfused {1e3 * seconds[False]:.3f} ms, fused {1e3 * seconds[True]:.3f} ms")
        for name, a, b in zip(("positions", "std", "velocities", "velocity variance"), out[True], out[False]):
            print(f"  {name}: max |fused - unfused| = {np.max(np.abs(a - b)):.2e}")
        dq = np.minimum(np.linalg.norm(out[True][4] - out[False][4], axis=1), np.linalg.norm(out[True][4] + out[False][4], axis=1))
        print(f"  orientations: max |fused - unfused| = {dq.max():.2e}")
        print(f"  det J_phi in [{info['det_vel'].min():.3f}, {info['det_vel'].max():.3f}] (<= 0: the map folds there); "
              f"smallest eigenvalue gap of the closest rotation {info['ori_gap'].min():.3f} (0: not unique)")
    return dict(fused=out[True], unfused=out[False], seconds=seconds, info=info)


if __name__ == "__main__":
    main()
