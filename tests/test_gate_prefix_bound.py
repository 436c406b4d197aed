"""The inequality behind the early exit of the chi2 gates (ekf_device.hpp gate_factor_chi2): the blocked left-looking Cholesky of [S; v']
finishes 16 entries of z = L^-1 v per block column, chi2 = z'z is a sum of squares, so its prefix after any block column is a lower bound
of chi2 -- a track whose prefix is above the threshold (by the margin 2^-20) is rejected whatever the remaining blocks hold. Restated in
numpy, in the kernel's order of operations (update of the block column by the finished ones, factor of the diagonal block, panel
solve), on random symmetric positive definite S of 20 .. 84 rows."""
import numpy as np

MARGIN = 1.0 + 2.0 ** -20


def _blocked_prefixes(S, v):
    """Left-looking blocked Cholesky of T = [S; v'] by 16-column blocks: the prefix of z'z behind every block column."""
    nr = len(v)
    T = np.vstack([np.tril(S), v[None, :]])
    prefixes, prefix = [], 0.0
    for j0 in range(0, nr, 16):
        w = min(16, nr - j0)
        if j0 > 0:
            T[j0:, j0:j0 + w] -= T[j0:, :j0] @ T[j0:j0 + w, :j0].T
        L = np.linalg.cholesky(T[j0:j0 + w, j0:j0 + w] + np.tril(T[j0:j0 + w, j0:j0 + w], -1).T)
        T[j0:j0 + w, j0:j0 + w] = L
        T[j0 + w:, j0:j0 + w] = np.linalg.solve(L, T[j0 + w:, j0:j0 + w].T).T            # rows below the block, row nr (v') included
        for c in range(w):
            prefix += T[nr, j0 + c] ** 2
        prefixes.append(prefix)
    return np.array(prefixes)


def _cases():
    rng = np.random.default_rng(20261)
    for _ in range(200):
        nr = int(rng.integers(20, 85))
        A = rng.normal(size=(nr, nr + 8))
        S = A @ A.T / nr + np.diag(rng.uniform(0.01, 1.0, nr))
        S = 0.5 * (S + S.T)
        yield nr, S, rng.normal(size=nr) * rng.choice([0.1, 1.0, 3.0])


def test_prefix_of_chi2_is_a_lower_bound_and_the_margin_rule_never_exits_an_inlier():
    exits, blocks_run, blocks_all = 0, 0, 0
    for nr, S, v in _cases():
        pre = _blocked_prefixes(S, v)
        assert len(pre) == (nr + 15) // 16
        assert np.all(np.diff(pre) >= 0.0)                                               # never decreases
        chi2 = float(v @ np.linalg.solve(S, v))
        assert abs(pre[-1] - chi2) <= 1e-12 * chi2, (nr, pre[-1], chi2)
        # thresholds around the final value and around every prefix: the rule (checked behind every block column but the last) may only
        # exit where the full sum is above the threshold
        for thr in np.concatenate([pre * (1 - 1e-9), pre * (1 + 1e-9), pre / MARGIN, [chi2 * 2.0, chi2 * 0.5]]):
            fired = np.nonzero(pre[:-1] > thr * MARGIN)[0]
            if len(fired):
                assert pre[-1] > thr, (nr, thr, pre)
                exits += 1
                blocks_run += int(fired[0]) + 1
            else:
                blocks_run += len(pre)
            blocks_all += len(pre)
    assert exits > 0 and blocks_run < blocks_all                                         # (the rule does fire on these inputs)
