"""CPU: the host half that track and register share (sgnn_amd/_gn.py) against the restatement of tests/track_ref.py:
the exponential, the layout and the solve of one system, the step over B transforms, and the rows of a record table.
No GPU and no kernels."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import track_ref as T  # noqa: E402
from sgnn_amd import _gn  # noqa: E402


def system(seed, n=200, scale=1.0):
    """A 32-entry system from n random rows of J and residuals: positive definite, well conditioned."""
    rng = np.random.default_rng(seed)
    J, r = rng.normal(size=(n, 6)) * scale, rng.normal(size=n) * 0.01
    a = J.T @ J
    return np.concatenate([a[np.triu_indices(6)], J.T @ r, [r @ r, n, 0, 0, 0]])


def test_se3_exp_against_the_series():
    """The three branches of the closed form: below the 1e-8 switch, a turn just short of pi, and a generic twist; the
    bound is the one test_track_ref holds track_ref.exp_se3 to."""
    axis = np.array([2.0, -1.0, 2.0]) / 3.0
    for xi in ([3e-9, -2e-9, 1e-9, 0.3, -0.2, 0.5], np.concatenate([axis * (np.pi - 1e-6), [0.4, 0.1, -0.3]]),
               [0.3, -0.2, 0.5, 1.0, 2.0, 3.0]):
        xi = np.array(xi)
        err = np.abs(_gn.se3_exp(xi) - T.exp_series(xi)).max()
        print('|omega| = %.3g: %.3g' % (np.linalg.norm(xi[:3]), err))
        assert err < 1e-14


def test_unpack_and_solve_step_against_the_restatement():
    good = system(0)
    few = system(1, n=63)                                                   # N < min_pairs = 64
    indefinite = good.copy()
    indefinite[0] = -good[0]                                                # A[0, 0] < 0: no Cholesky factor
    poisoned = good.copy()
    poisoned[23] = np.nan                                                   # an entry of g
    for name, s, solvable in (('good', good, True), ('few', few, False), ('indefinite', indefinite, False),
                              ('poisoned', poisoned, False)):
        for mine, ref in zip(_gn.unpack(s), T.unpack(s)):
            assert np.array_equal(mine, ref, equal_nan=True), name
        xi, n, e = _gn.solve_step(s, 64)
        ref = T.step(s, 64)
        assert (n, e) == (int(s[_gn.N_INDEX]), float(s[_gn.E_INDEX])), name
        assert (xi is not None) == solvable and (ref is not None) == solvable, name
        if solvable:
            a, g, _, _ = T.unpack(s)
            assert np.array_equal(xi, ref) and np.abs(a @ xi + g).max() <= 1e-12 * np.abs(g).max()
    assert _gn.solve_step(few, 63)[0] is not None                            # the pair count alone turned it down


def test_steps_over_three_records():
    """Record 1 fails on the second of three calls: it ends on its guess, stays dead whatever its later systems hold,
    and its history stops; the others are what they are when they run alone."""
    guess = np.stack([_gn.se3_exp(np.arange(6) * 0.01 * (b + 1)) for b in range(3)])
    calls = [np.stack([system(10 * c + b, scale=3.0) for b in range(3)]) for c in range(3)]
    calls[1][1] = system(99, n=10)
    run = _gn.Steps(guess, 64)
    for systems in calls:
        run.step(systems)
    assert list(run.alive) == [True, False, True]
    assert np.array_equal(run.T[1], guess[1]) and np.isnan(run.rmse[1])
    assert run.history[1] == [200, 10] and run.pairs[1] == 10
    for b in range(3):
        alone = _gn.Steps(guess[b:b + 1], 64)
        for systems in calls:
            alone.step(systems[b:b + 1])
        assert np.array_equal(alone.T[0], run.T[b]) and alone.alive[0] == run.alive[b]
        assert alone.pairs[0] == run.pairs[b] and alone.history[0] == run.history[b]
        assert np.array_equal(alone.rmse[0], run.rmse[b], equal_nan=True)
    assert run.history[0] == run.history[2] == [200, 200, 200]
    assert not np.array_equal(run.T[0], guess[0]) and run.rmse[0] == np.sqrt(calls[2][0][27] / 200)


def test_record_rows():
    rows = np.random.default_rng(5).normal(size=(4, 12)) * 1e3
    rows[1, 9] = 1e39                                                       # finite in fp64, inf in fp32
    rows[3, 0] = np.inf
    out = _gn.record_rows(rows)
    assert out.dtype == np.float32 and out.shape == rows.shape
    assert np.isnan(out[1]).all() and np.isnan(out[3]).all()
    for b in (0, 2):
        assert np.array_equal(out[b], rows[b].astype(np.float32))
    assert np.isnan(_gn.record_rows(rows, np.array([False, True, True, True]))[0]).all()
    assert np.array_equal(_gn.record_rows(rows[:1]), rows[:1].astype(np.float32))
