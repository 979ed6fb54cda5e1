"""gpt_apply_inverse (csrc/gpt_api.hip, _lib.Handle.apply_inverse): (K + sigma^2 I)^-1 R for caller-supplied columns through the
launches that compute alpha in the fit (launch_alpha, csrc/gpt_fit.hip), four columns per pass.

  1. R = Y is the exported alpha, bit for bit.
  2. C in {1, 4, 5, 9}: every column equals its own one-column call, bit for bit (passes, the padded last pass).
  3. N in {5, 512, 513} (one padded block, a full one, one row past it): against W^T (W R) restated in numpy from the exported
     inverse factor, error / max(e_oracle, N 2^-53 |out|_max) <= 32, e_oracle the restatement against its longdouble twin (the rule
     of tests/test_fold_scan.py).
  4. refusals."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

LD = np.longdouble


def _fit(N, D=2, O=2, seed=0, ktype=0, dtype=None):
    from gaussian_process_transportation_amd import _lib
    rs = np.random.RandomState(seed)
    X = rs.uniform(-2.0, 2.0, (N, D))
    Y = np.sin(X @ rs.standard_normal((D, O))) + 0.05 * rs.standard_normal((N, O))
    h = _lib.Handle(0)
    if dtype is not None:
        h.set_dtype(dtype)
    h.fit(X, Y, np.full(D, 0.7), 0.8, 0.01, 1e-10, ktype)
    return h, X, Y


@pytest.mark.gpu
@pytest.mark.parametrize("N,O", [(5, 2), (130, 3), (513, 5)])
def test_targets_give_alpha(N, O):
    """1.  O = 5: alpha of the fit itself takes two passes."""
    h, _, Y = _fit(N, O=O)
    got = h.apply_inverse(Y)
    assert_array_equal(got, h.export(want_L=False)[1])
    assert_array_equal(h.apply_inverse(Y[:, 0]), got[:, 0])       # (N,) in, (N,) out
    h.close()


@pytest.mark.gpu
def test_columns_do_not_depend_on_each_other():
    """2."""
    h, _, _ = _fit(130, seed=1)
    R = np.random.RandomState(2).standard_normal((130, 9))
    R[:, 3] = 0.0
    R[:, 6] *= 1e150
    single = [h.apply_inverse(np.ascontiguousarray(R[:, c:c + 1]))[:, 0] for c in range(9)]
    for C in (1, 4, 5, 9):
        got = h.apply_inverse(np.ascontiguousarray(R[:, :C]))
        assert got.shape == (130, C)
        for c in range(C):
            assert_array_equal(got[:, c], single[c], err_msg=f"C = {C}, column {c}")
    rev = h.apply_inverse(np.ascontiguousarray(R[:, ::-1]))
    for c in range(9):
        assert_array_equal(rev[:, 8 - c], single[c], err_msg=f"reversed, column {c}")
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [5, 512, 513])
def test_against_the_exported_factor(N):
    """3."""
    h, _, _ = _fit(N, seed=N)
    W = np.tril(h.export_inverse_factor())
    R = np.random.RandomState(7).standard_normal((N, 5))
    got = h.apply_inverse(R)
    ref64 = W.T @ (W @ R)
    Wl, Rl = W.astype(LD), R.astype(LD)
    ref = Wl.T @ (Wl @ Rl)
    e_oracle = float(np.max(np.abs(ref64 - ref)))
    err = float(np.max(np.abs(got - ref)))
    floor = N * 2.0 ** -53 * float(np.max(np.abs(got)))
    print(f"ratio apply_inverse N={N} {err / max(e_oracle, floor):.2f}   (gpu {err:.2e}, oracle {e_oracle:.2e}, floor {floor:.2e})")
    assert err <= 32 * max(e_oracle, floor)
    h.close()


@pytest.mark.gpu
def test_refusals():
    """4."""
    from gaussian_process_transportation_amd import _lib
    h, X, Y = _fit(20)
    with pytest.raises(ValueError, match="one row per training point"):
        h.apply_inverse(np.zeros((19, 2)))
    with pytest.raises(ValueError, match="one row per training point"):
        h.apply_inverse(np.zeros((20, 2, 1)))
    lib, dp = _lib.load(), _lib.dptr
    out = np.full((20, 2), -7.0)
    assert lib.gpt_apply_inverse(h._h, dp(Y), -1, dp(out)) == _lib.GPT_E_ARG and "C must be" in _lib.last_error()
    assert lib.gpt_apply_inverse(h._h, None, 2, dp(out)) == _lib.GPT_E_ARG and "NULL" in _lib.last_error()
    assert lib.gpt_apply_inverse(h._h, dp(Y), 2, None) == _lib.GPT_E_ARG
    assert lib.gpt_apply_inverse(None, dp(Y), 2, dp(out)) == _lib.GPT_E_ARG
    assert lib.gpt_apply_inverse(h._h, None, 0, None) == _lib.GPT_OK
    assert np.all(out == -7.0)
    bare = _lib.Handle(0)
    assert lib.gpt_apply_inverse(bare._h, dp(Y), 2, dp(out)) == _lib.GPT_E_STATE and "not fitted" in _lib.last_error()
    bare.factor_copy_from(h)                                      # a replica holds the model, not the factor
    assert lib.gpt_apply_inverse(bare._h, dp(Y), 2, dp(out)) == _lib.GPT_E_ARG and "inverse factor" in _lib.last_error()
    bare.close()
    f32, _, Y32 = _fit(20, dtype=_lib.GPT_F32)
    assert lib.gpt_apply_inverse(f32._h, dp(Y32), 2, dp(out)) == _lib.GPT_E_ARG and "fp64 models only" in _lib.last_error()
    f32.close()
    assert np.all(out == -7.0)
    assert_array_equal(h.apply_inverse(Y), h.export(want_L=False)[1])     # the handle serves on after the refusals
    h.close()
