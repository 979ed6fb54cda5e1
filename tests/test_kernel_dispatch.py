"""Every launch case of the prediction side is reached and returns right numbers: element type x kernel type x coordinate width
x requested outputs, at the smallest model there is (N = 40: one 512-row i-block) with M = 70 queries, so that queries x
columns passes one 64-column block.  Which kernel a case takes is decided in csrc/gpt_dispatch.h and gpt_kvar.h
(launch_kvar); a case whose kernel lacked its dynamic-LDS opt-in would fail at launch, and the call would return an error.

References: oracle/gp_oracle.py (mean and variance of every kernel type, RBF derivatives) and the numpy Matern posterior of
tests/test_matern_derivatives.py.  Bounds are those of the tests that already hold these outputs: 1e-5 of the array scale for
fp64 (test_ragged_shapes_vs_oracle, test_input_dimension_beyond_three_vs_oracle), 1e-8 for fp64 Matern 3/2 and 5/2 models
(test_matern_derivatives.test_outputs_against_numpy), 2e-4 for fp32 (test_fp32_exact_gp_model), and 2e-4 of the prior
derivative variance for the fp32 Matern Jvar (test_matern_derivatives.test_fp32_model_against_fp64)."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests.conftest import assert_parity
from tests.test_matern_derivatives import G0, np_posterior

pytestmark = pytest.mark.gpu

N, M = 40, 70
C, NOISE, JIT = 0.5, 1e-2, 1e-10
KINDS = ("rbf", "matern12", "matern32", "matern52")          # by kernel_type code (GPT_KERNEL_*)
NU = {2: 1.5, 3: 2.5}
# D: rows of 4 | DERIV4 and fused 8 | fused 8 | DERIV8 and fused 16 on rows of 8 | rows of 16
DIMS = (2, 4, 6, 8, 12)
# variance alone (1 column per query) | k_mean_jac alone | Jacobian variance alone, twice | fused with the cross products | fused without
REQUESTS = (dict(var=True), dict(mean=True, J=True), dict(J=True, Jvar=True), dict(Jvar=True), dict(J=True, Jvar=True, dvar=True),
            dict(var=True, Jvar=True))


def length_scales(D):
    return np.linspace(0.4, 0.6, D)


@functools.lru_cache(maxsize=None)
def problem(kt, D, O=2, n_queries=M):
    """(X, Y, Xq, reference outputs) from a fixed seed, read-only and shared by the cases that use them.  Checked here, on
    the CPU: the Gram matrix is well-conditioned (cond <= (c N + noise) / noise ~ 2e3, so fp64 leaves ~1e-12 to the
    reference) and every reference output is finite."""
    from oracle import gp_oracle as orc
    rng = np.random.default_rng(4000 + D)
    X = rng.uniform(0, 1, (N, D))
    Y = np.sin(3 * X[:, :1] + np.arange(O)[None, :]) + 0.01 * rng.standard_normal((N, O))
    Xq = rng.uniform(-0.1, 1.1, (n_queries, D))
    ls, kind = length_scales(D), KINDS[kt]
    K = orc.kernel_train(X, C, ls, NOISE + JIT, kind)
    assert np.linalg.cond(K) < 1e4
    L, a = orc.gpr_fit(X, Y, C, ls, NOISE, JIT, kind)
    mean, std = orc.gpr_predict(Xq, X, L, a, C, ls, NOISE, return_std=True, kind=kind)
    ref = {"mean": mean.reshape(n_queries, O), "var": (std if std.ndim == 1 else std[:, 0]) ** 2}
    if kt == 0:
        o = orc.GaussianProcessOracle(C, ls, NOISE, JIT).fit(X, Y)
        J, Jv = o.derivative(Xq, return_var=True)
        ref.update(J=J, Jvar=Jv[:, 0, :], dvar=o.derivative_of_variance(Xq))
    elif kt in NU:
        _, _, J, Jvar, dvar = np_posterior(Xq, X, Y, C, ls, NU[kt], NOISE, JIT)
        ref.update(J=J, Jvar=Jvar, dvar=dvar)
    for v in (X, Y, Xq, *ref.values()):
        assert np.all(np.isfinite(v))
        v.setflags(write=False)
    return X, Y, Xq, ref


def on_fresh_thread(fn):
    """gpt_last_error is per thread and a successful call leaves it alone: on a new thread it starts empty, so that `empty
    after the call` says something about this call."""
    with ThreadPoolExecutor(max_workers=1) as ex:
        return ex.submit(fn).result()


def fitted(kt, D, dtype, X, Y):
    from gaussian_process_transportation_amd import _lib
    h = _lib.Handle(0)
    h.set_dtype(dtype)
    h.set_matern_derivatives(True)
    h.fit(X, Y, length_scales(D), C, NOISE, JIT, kernel_type=kt)
    assert _lib.last_error() == ""
    return h


def predict(h, Xq, **flags):
    from gaussian_process_transportation_amd import _lib
    out = h.predict_all(Xq, **flags)                 # raises unless the call returned GPT_OK
    assert _lib.last_error() == "", flags
    return {k: v for k, v in out.items() if v is not None}


def check(out, ref, kt, D, dtype, what):
    from gaussian_process_transportation_amd import _lib
    for k, a in out.items():
        assert a.dtype == (np.float32 if dtype == _lib.GPT_F32 else np.float64)
        print(f"{what} {k}: max-norm relative error {np.max(np.abs(a - ref[k])) / np.max(np.abs(ref[k])):.3e}")
        if dtype == _lib.GPT_F32 and kt in NU and k == "Jvar":
            prior = C * G0[NU[kt]] * float(np.max(1.0 / length_scales(D) ** 2))
            assert np.max(np.abs(a - ref[k])) < 2e-4 * prior, what
        else:
            tol = 2e-4 if dtype == _lib.GPT_F32 else (1e-8 if kt in NU else 1e-5)
            assert_parity(a, ref[k], tol, f"{what} {k}")


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("kt", range(4))
@pytest.mark.parametrize("dtype", [0, 1], ids=["fp64", "fp32"])
def test_every_launch_case_against_the_oracle(dtype, kt, D, monkeypatch):
    from gaussian_process_transportation_amd import _lib
    X, Y, Xq, ref = problem(kt, D)

    def run():
        monkeypatch.delenv("GPT_VAR_DIAG_HALF", raising=False)
        h = fitted(kt, D, dtype, X, Y)
        # Matern 1/2 is not differentiable at the sources: mean and variance only
        for flags in (REQUESTS if kt != 1 else (dict(var=True), dict(mean=True))):
            out = predict(h, Xq, **flags)
            check(out, ref, kt, D, dtype, f"{KINDS[kt]} D={D} {sorted(flags)}")
            if dtype == _lib.GPT_F64 and set(flags) & {"var", "Jvar", "dvar"}:
                # the default took the HALF kernels where they exist; the plain ones must agree to the bit
                monkeypatch.setenv("GPT_VAR_DIAG_HALF", "0")
                plain = predict(h, Xq, **flags)
                monkeypatch.delenv("GPT_VAR_DIAG_HALF")
                for k, a in out.items():
                    assert np.array_equal(a, plain[k]), (k, flags)
        if kt == 1:
            for flags in (dict(J=True), dict(Jvar=True), dict(dvar=True), dict(mean=True, J=True)):
                with pytest.raises(ValueError, match="Matern 1/2"):
                    h.predict_all(Xq, **flags)
        h.close()

    on_fresh_thread(run)


@pytest.mark.parametrize("with_J", [False, True])
@pytest.mark.parametrize("O", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("dtype", [0, 1], ids=["fp64", "fp32"])
def test_mean_and_jacobian_by_number_of_outputs(dtype, O, with_J):
    """k_mean_jac takes up to four outputs per pass; five make a second pass of four."""
    X, Y, Xq, ref = problem(0, 2, O)

    def run():
        h = fitted(0, 2, dtype, X, Y)
        out = predict(h, Xq, mean=True, J=with_J)
        assert out["mean"].shape == (M, O) and ("J" in out) == with_J
        check(out, ref, 0, 2, dtype, f"O={O}")
        h.close()

    on_fresh_thread(run)


@pytest.mark.parametrize("dtype", [0, 1], ids=["fp64", "fp32"])
def test_mean_alone_of_many_queries(dtype):
    """From 32768 queries on, the mean alone of a D <= 3 model takes the kernel with four queries per wave; 5 past it
    leave a wave with one query."""
    X, Y, Xq, ref = problem(0, 2, 2, 32768 + 5)

    def run():
        h = fitted(0, 2, dtype, X, Y)
        check(predict(h, Xq, mean=True), ref, 0, 2, dtype, "M=32773")
        h.close()

    on_fresh_thread(run)
