"""numpy restatement of the reference's five-point RANSAC (doRansac5 without Theia) and of the hybrid RANSAC2 / RANSAC5
selection (src/tracker/ransac_pipeline.cpp:95-195, 274-397; five_point.cpp; ptsetreg.{hpp,cpp}).

Test infrastructure only (imported by the tests, never by the product). It states the algorithm the device kernel
(hybvio_amd/csrc/ransac5.hip) runs, operation by operation in binary64, vectorised over hypotheses:
  - cv::RNG((uint64)-1) multiply-with-carry and getSubset's redraw of duplicates (no checkSubset for the EM callback)
  - the null space of the 5 x 9 epipolar constraint matrix from a Householder QR of its 9 x 5 transpose (the reference's
    Jacobi SVD fills its extra basis vectors from an internal RNG, so any orthonormal basis is as faithful)
  - the 10 x 20 cubic-constraint matrix derived here by polynomial arithmetic on E(x, y, z) = xX + yY + zZ + W:
    det(E) and E E^T E - tr(E E^T) E / 2, columns in Nister's monomial order (the order of the reference after its `perm`)
  - Gaussian elimination with partial pivoting of the left 10 x 10 block, solved against the right block
  - the 3 x 13 matrix B and its degree-10 determinant by polynomial convolution
  - cv::solvePoly's Durand-Kerner iteration (start (0.4 + 0.9i)^k, in-place updates, <= 300 sweeps, stop when no root moved)
    as remembered from OpenCV 4.x; roots with |im| > 1e-10 dropped
  - the null vector of B(z) from the largest cross product of two of its rows (the reference: SVD::solveZ), |w| < 1e-10 dropped
  - the float Sampson error, `err <= (float)(thr^2)`, the strict `goodCount > max(best, 4)` rule and RANSACUpdateNumIters.
Every elementwise numpy operation rounds once, as the kernel does (built without FMA contraction); sums are written as
explicit sequential chains so that both sides add in the same order.
"""
from __future__ import annotations

import math

import numpy as np

f64 = np.float64
DBL_EPSILON = float(np.finfo(np.float64).eps)
DBL_MIN = float(np.finfo(np.float64).tiny)
MODEL_POINTS = 5
DK_MAX_ITERS = 300
TRACKED, RANSAC_OUTLIER = 0, 3
TYPE_SKIPPED, TYPE_R2, TYPE_R5 = 0, 1, 3


class Params:
    """tracker.* parameters of the hybrid path (codegen/parameter_definitions.c:268-282)."""

    def __init__(self, ransac5Prob=0.999, ransac5Threshold=2.0, ransacMaxIters=75, ransac2InliersToSkipRansac5=0.9,
                 ransacMinInlierFraction=0.3, ransac2InliersOverRansac5Needed=0.9):
        self.ransac5Prob, self.ransac5Threshold, self.ransacMaxIters = ransac5Prob, ransac5Threshold, ransacMaxIters
        self.ransac2InliersToSkipRansac5 = ransac2InliersToSkipRansac5
        self.ransacMinInlierFraction = ransacMinInlierFraction
        self.ransac2InliersOverRansac5Needed = ransac2InliersOverRansac5Needed


# ---- cv::RNG and getSubset ----
def rng_subsets(count: int, iters: int) -> np.ndarray:
    """The 5-index subsets of `iters` consecutive getSubset calls on a fresh cv::RNG((uint64)-1) -> [iters, 5] int32."""
    state = 0xFFFFFFFFFFFFFFFF
    out = np.zeros((iters, MODEL_POINTS), np.int32)
    for it in range(iters):
        for i in range(MODEL_POINTS):
            while True:
                state = ((state & 0xFFFFFFFF) * 4164903690 + (state >> 32)) & 0xFFFFFFFFFFFFFFFF
                v = (state & 0xFFFFFFFF) % count
                if v not in out[it, :i]:
                    break
            out[it, i] = v
    return out


def update_num_iters(p: float, ep: float, model_points: int, max_iters: int) -> int:
    """RANSACUpdateNumIters (ptsetreg.cpp:58-79); cvRound rounds half to even."""
    p = min(max(p, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    denom = 1.0 - math.pow(1.0 - ep, model_points)
    if denom < DBL_MIN:
        return 0
    num = math.log(num)
    denom = math.log(denom)
    return max_iters if (denom >= 0 or -num >= max_iters * (-denom)) else int(np.rint(num / denom))


# ---- monomials: linear [x, y, z, 1], quadratic (pairs a <= b), cubic in Nister's order ----
def _exp(mono):
    e = [0, 0, 0]
    for v in mono:
        if v < 3:
            e[v] += 1
    return tuple(e)


QUAD = [(a, b) for a in range(4) for b in range(a, 4)]
CUBIC_EXP = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
             (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0)]
IDX2 = np.zeros((4, 4), np.int32)
for _q, (_a, _b) in enumerate(QUAD):
    IDX2[_a, _b] = IDX2[_b, _a] = _q
IDX3 = np.zeros((10, 4), np.int32)          # quadratic monomial q times linear monomial b -> cubic column
for _q, (_a, _b) in enumerate(QUAD):
    for _c in range(4):
        IDX3[_q, _c] = CUBIC_EXP.index(_exp((_a, _b, _c)))


def _sumchain(terms):
    s = terms[0]
    for t in terms[1:]:
        s = s + t
    return s


# ---- the minimal solver, vectorised over hypotheses ----
def null_basis(x1, y1, x2, y2):
    """x*, y* [H, 5] -> N [H, 9, 4]: columns X, Y, Z, W (entries = E row-major) spanning the null space of the 5 x 9 matrix."""
    H = x1.shape[0]
    one = np.ones(H)
    M = [[None] * 5 for _ in range(9)]      # M = Q^T, M[i][k] = entry i of point k's constraint row
    for k in range(5):
        a, b, c, d = x1[:, k], y1[:, k], x2[:, k], y2[:, k]
        row = [a * c, b * c, c, a * d, b * d, d, a, b, one]
        for i in range(9):
            M[i][k] = row[i]
    P = [[np.full(H, 1.0 if i == c else 0.0) for c in range(9)] for i in range(9)]   # P = H4 ... H0, column by column
    for k in range(5):
        s = M[k][k] * M[k][k]
        for i in range(k + 1, 9):
            s = s + M[i][k] * M[i][k]
        nrm = np.sqrt(s)
        alpha = np.where(M[k][k] >= 0, -nrm, nrm)
        v = [None] * 9
        v[k] = M[k][k] - alpha
        for i in range(k + 1, 9):
            v[i] = M[i][k]
        vv = v[k] * v[k]
        for i in range(k + 1, 9):
            vv = vv + v[i] * v[i]
        ok = vv > 0
        vvs = np.where(ok, vv, 1.0)

        def reflect(col):
            d = v[k] * col[k]
            for i in range(k + 1, 9):
                d = d + v[i] * col[i]
            f = (d + d) / vvs
            for i in range(k, 9):
                col[i] = np.where(ok, col[i] - f * v[i], col[i])

        for j in range(k + 1, 5):
            col = [M[i][j] for i in range(9)]
            reflect(col)
            for i in range(9):
                M[i][j] = col[i]
        for c in range(9):
            col = [P[i][c] for i in range(9)]
            reflect(col)
            for i in range(9):
                P[i][c] = col[i]
    N = np.empty((H, 9, 4))
    for j in range(4):
        for i in range(9):
            N[:, i, j] = P[5 + j][i]
    return N


def coeff_matrix(N):
    """N [H, 9, 4] -> A [H, 10, 20]: rows 0..8 = (E E^T E - tr(E E^T) E / 2)_ij (row-major), row 9 = det(E)."""
    H = N.shape[0]
    E = lambda r, c: [N[:, 3 * r + c, m] for m in range(4)]     # linear polynomial of entry (r, c)
    EEt = {}
    for i in range(3):
        for k in range(3):
            acc = [np.zeros(H) for _ in range(10)]
            for m in range(3):
                p, q = E(i, m), E(k, m)
                for a in range(4):
                    for b in range(4):
                        t = IDX2[a, b]
                        acc[t] = acc[t] + p[a] * q[b]
            EEt[i, k] = acc
    half_tr = [0.5 * ((EEt[0, 0][t] + EEt[1, 1][t]) + EEt[2, 2][t]) for t in range(10)]
    A = np.zeros((H, 10, 20))
    for i in range(3):
        for j in range(3):
            acc = [np.zeros(H) for _ in range(20)]
            for k in range(3):
                Mq = [EEt[i, k][t] - half_tr[t] for t in range(10)] if i == k else EEt[i, k]
                e = E(k, j)
                for t in range(10):
                    for b in range(4):
                        c = IDX3[t, b]
                        acc[c] = acc[c] + Mq[t] * e[b]
            for c in range(20):
                A[:, 3 * i + j, c] = acc[c]

    def minor(p, q, r, s):
        acc = [np.zeros(H) for _ in range(10)]
        for a in range(4):
            for b in range(4):
                acc[IDX2[a, b]] = acc[IDX2[a, b]] + p[a] * q[b]
        for a in range(4):
            for b in range(4):
                acc[IDX2[a, b]] = acc[IDX2[a, b]] - r[a] * s[b]
        return acc

    m0 = minor(E(1, 1), E(2, 2), E(1, 2), E(2, 1))
    m1 = minor(E(1, 0), E(2, 2), E(1, 2), E(2, 0))
    m2 = minor(E(1, 0), E(2, 1), E(1, 1), E(2, 0))
    acc = [np.zeros(H) for _ in range(20)]
    for sgn, e, m in ((1, E(0, 0), m0), (-1, E(0, 1), m1), (1, E(0, 2), m2)):
        for a in range(4):
            for t in range(10):
                c = IDX3[t, a]
                acc[c] = acc[c] + e[a] * m[t] if sgn > 0 else acc[c] - e[a] * m[t]
    for c in range(20):
        A[:, 9, c] = acc[c]
    return A


def eliminate(A):
    """Gaussian elimination with partial pivoting (first maximum of |a|) of the left block, back-substitution of the right:
    A [H, 10, 20] -> (X [H, 10, 10] = left^-1 right, ok [H] = no zero pivot)."""
    A = A.copy()
    H = A.shape[0]
    ar = np.arange(H)
    ok = np.ones(H, bool)
    for k in range(10):
        p = np.full(H, k)
        best = np.abs(A[:, k, k])
        for r in range(k + 1, 10):
            a = np.abs(A[:, r, k])
            gt = a > best
            best = np.where(gt, a, best)
            p = np.where(gt, r, p)
        rowk = A[ar, k].copy()
        A[ar, k] = A[ar, p]
        A[ar, p] = rowk
        piv = A[:, k, k]
        ok &= piv != 0
        pivs = np.where(piv != 0, piv, 1.0)
        for r in range(k + 1, 10):
            l = A[:, r, k] / pivs
            for c in range(k + 1, 20):
                A[:, r, c] = A[:, r, c] - l * A[:, k, c]
    for c in range(10, 20):
        for i in range(9, -1, -1):
            s = A[:, i, c]
            for j in range(i + 1, 10):
                s = s - A[:, i, j] * A[:, j, c]
            A[:, i, c] = s / np.where(A[:, i, i] != 0, A[:, i, i], 1.0)
    return A[:, :, 10:], ok


B_POS1 = [1, 2, 3, 5, 6, 7, 9, 10, 11, 12]     # row (2i+4) of the right block: x (z^2, z, 1), y (z^2, z, 1), 1 (z^3 .. 1)
B_POS2 = [0, 1, 2, 4, 5, 6, 8, 9, 10, 11]      # row (2i+5), multiplied by z


def b_matrix(X):
    """X [H, 10, 10] -> B [H, 3, 13]: row i = <2i+4> - z <2i+5>, coefficients of x (z^3..1), y (z^3..1), 1 (z^4..1)."""
    H = X.shape[0]
    B = np.zeros((H, 3, 13))
    for i in range(3):
        r1 = np.zeros((H, 13))
        r2 = np.zeros((H, 13))
        for m in range(10):
            r1[:, B_POS1[m]] = X[:, 2 * i + 4, m]
            r2[:, B_POS2[m]] = X[:, 2 * i + 5, m]
        B[:, i] = r1 - r2
    return B


def _asc(B, j, part):
    if part == 0:
        return [B[:, j, 3 - i] for i in range(4)]
    if part == 1:
        return [B[:, j, 7 - i] for i in range(4)]
    return [B[:, j, 12 - i] for i in range(5)]


def _conv_into(acc, p, q, sign):
    for k in range(len(acc)):
        for i in range(len(p)):
            j = k - i
            if 0 <= j < len(q):
                acc[k] = acc[k] + p[i] * q[j] if sign > 0 else acc[k] - p[i] * q[j]


def det_poly(B):
    """det B(z) -> c [H, 11], c[k] = coefficient of z^k."""
    H = B.shape[0]
    bx = [_asc(B, j, 0) for j in range(3)]
    by = [_asc(B, j, 1) for j in range(3)]
    bc = [_asc(B, j, 2) for j in range(3)]

    def minor(p, q, r, s, deg):
        acc = [np.zeros(H) for _ in range(deg + 1)]
        _conv_into(acc, p, q, 1)
        _conv_into(acc, r, s, -1)
        return acc

    m0 = minor(by[1], bc[2], bc[1], by[2], 7)
    m1 = minor(bx[1], bc[2], bc[1], bx[2], 7)
    m2 = minor(bx[1], by[2], by[1], bx[2], 6)
    c = [np.zeros(H) for _ in range(11)]
    _conv_into(c, bx[0], m0, 1)
    _conv_into(c, by[0], m1, -1)
    _conv_into(c, bc[0], m2, 1)
    return np.stack(c, axis=1)


def solve_poly(c, max_iters=DK_MAX_ITERS):
    """cv::solvePoly on real coefficients c [H, 11] (ascending) -> (re [H, 10], im [H, 10], n [H] roots, sweeps [H]).
    Leading coefficients with |c_n| <= DBL_EPSILON are dropped (n >= 1); only roots 0..n-1 are meaningful."""
    H = c.shape[0]
    n = np.full(H, 10)
    for k in range(10, 1, -1):
        n = np.where((n == k) & ~(np.abs(c[:, k]) > DBL_EPSILON), k - 1, n)
    re, im = np.zeros((H, 10)), np.zeros((H, 10))
    sweeps = np.zeros(H, np.int32)
    for nn in np.unique(n):
        sel = np.nonzero(n == nn)[0]
        d = [c[sel, nn - j] for j in range(nn + 1)]           # Horner order: c_n, c_{n-1}, ..., c_0
        rr, ri = _dk(d, int(nn), max_iters, sweeps, sel)
        re[sel, :nn], im[sel, :nn] = rr, ri
    return re, im, n, sweeps


def _dk(d, n, max_iters, sweeps_out, sel):
    h = d[0].shape[0]
    rr, ri = [None] * n, [None] * n
    pr, pi = np.ones(h), np.zeros(h)
    for i in range(n):
        rr[i], ri[i] = pr, pi
        pr, pi = pr * 0.4 - pi * 0.9, pr * 0.9 + pi * 0.4
    active = np.ones(h, bool)
    sweeps = np.full(h, max_iters, np.int32)
    for it in range(max_iters):
        md = np.zeros(h)
        for i in range(n):
            pr, pi = rr[i], ri[i]
            nr, ni = d[0], np.zeros(h)
            dr, di = d[0], np.zeros(h)
            for j in range(n):
                nr, ni = nr * pr - ni * pi, nr * pi + ni * pr
                nr, ni = nr + d[j + 1], ni + 0.0
                if j != i:
                    sr, si = pr - rr[j], pi - ri[j]
                    dr, di = dr * sr - di * si, dr * si + di * sr
            t = 1.0 / (dr * dr + di * di)
            qr = (nr * dr + ni * di) * t
            qi = ((-nr) * di + ni * dr) * t
            rr[i] = np.where(active, pr - qr, pr)
            ri[i] = np.where(active, pi - qi, pi)
            a = np.sqrt(qr * qr + qi * qi)
            md = np.where(md < a, a, md)
        stop = active & (md <= 0)
        sweeps[stop] = it + 1
        active &= ~stop
        if not active.any():
            break
    sweeps_out[sel] = sweeps
    return np.stack(rr, axis=1), np.stack(ri, axis=1)


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def models_from_roots(N, B, re, im, n, ok):
    """Back-substitution of every root -> (E [H, 10, 9], valid [H, 10]) in root order."""
    H = N.shape[0]
    E = np.zeros((H, 10, 9))
    valid = np.zeros((H, 10), bool)
    for r in range(10):
        z1 = re[:, r]
        z2 = z1 * z1
        z3 = z2 * z1
        z4 = z3 * z1
        rows = []
        for j in range(3):
            b = B[:, j]
            rows.append([((b[:, 0] * z3 + b[:, 1] * z2) + b[:, 2] * z1) + b[:, 3],
                         ((b[:, 4] * z3 + b[:, 5] * z2) + b[:, 6] * z1) + b[:, 7],
                         (((b[:, 8] * z4 + b[:, 9] * z3) + b[:, 10] * z2) + b[:, 11] * z1) + b[:, 12]])
        best, bs = _cross(rows[0], rows[1]), None
        bs = (best[0] * best[0] + best[1] * best[1]) + best[2] * best[2]
        for a, b in ((0, 2), (1, 2)):
            c = _cross(rows[a], rows[b])
            s = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
            gt = s > bs
            best = [np.where(gt, c[t], best[t]) for t in range(3)]
            bs = np.where(gt, s, bs)
        nrm = np.sqrt(bs)
        nz = nrm > 0
        nrms = np.where(nz, nrm, 1.0)
        w = [best[t] / nrms for t in range(3)]
        good = ok & (r < n) & ~(np.abs(im[:, r]) > 1e-10) & nz & ~(np.abs(w[2]) < 1e-10)
        w2 = np.where(good, w[2], 1.0)
        x, y = w[0] / w2, w[1] / w2
        e = [((N[:, i, 0] * x + N[:, i, 1] * y) + N[:, i, 2] * z1) + N[:, i, 3] for i in range(9)]
        s = _sumchain([e[i] * e[i] for i in range(9)])
        inv = 1.0 / np.where(good & (s > 0), np.sqrt(s), 1.0)
        for i in range(9):
            E[:, r, i] = e[i] * inv
        valid[:, r] = good
    return E, valid


def essential_kernel(x1, y1, x2, y2):
    """EMEstimatorCallback::runKernel on H 5-point samples [H, 5] -> (E [H, 10, 9], valid [H, 10], DK sweeps [H])."""
    N = null_basis(x1, y1, x2, y2)
    X, ok = eliminate(coeff_matrix(N))
    B = b_matrix(X)
    c = det_poly(B)
    re, im, n, sweeps = solve_poly(np.where(ok[:, None], c, 0.0))
    E, valid = models_from_roots(N, B, re, im, n, ok)
    return E, valid, np.where(ok, sweeps, 0)


def sampson_err(E, h1, h2):
    """computeError (five_point.cpp:374-400): E [..., 9] against points h* [n, 2] -> float32 [..., n]."""
    e = [E[..., i, None] for i in range(9)]
    a1, b1, a2, b2 = h1[:, 0], h1[:, 1], h2[:, 0], h2[:, 1]
    ex = [(e[3 * r] * a1 + e[3 * r + 1] * b1) + e[3 * r + 2] for r in range(3)]
    et = [(e[c] * a2 + e[3 + c] * b2) + e[6 + c] for c in range(2)]
    x2tex1 = (a2 * ex[0] + b2 * ex[1]) + ex[2]
    den = ((ex[0] * ex[0] + ex[1] * ex[1]) + et[0] * et[0]) + et[1] * et[1]
    return ((x2tex1 * x2tex1) / den).astype(np.float32)


# ---- the registrator run and doRansac5 ----
def normalize(c1, c2, cam1, cam2):
    """Camera::normalizePixel of both frames (camera.cpp:471-476) with the oracle cameras -> (h1 [m, 2], h2 [m, 2], index [m])."""
    h1, h2, idx = [], [], []
    for i in range(len(c1)):
        ok1, r1 = cam1.pixel_to_ray(float(np.float32(c1[i][0])), float(np.float32(c1[i][1])))
        ok2, r2 = cam2.pixel_to_ray(float(np.float32(c2[i][0])), float(np.float32(c2[i][1])))
        if ok1 and r1[2] > 0 and ok2 and r2[2] > 0:
            h1.append((r1[0] / r1[2], r1[1] / r1[2]))
            h2.append((r2[0] / r2[2], r2[1] / r2[2]))
            idx.append(i)
    return np.array(h1, f64).reshape(-1, 2), np.array(h2, f64).reshape(-1, 2), np.array(idx, np.int64)


def threshold(cam1_f: float, cam2_f: float, ransac5Threshold: float = 2.0) -> float:
    """ransac_pipeline.cpp:330: 2 * ransac5Threshold / (f1 + f2), f = (fx + fy) / 2."""
    return 2 * ransac5Threshold / (cam1_f + cam2_f)


class Run:
    """Result of one findEssentialMatRansacMaxIter call on m valid points."""
    mask: np.ndarray            # [m] uint8
    E: np.ndarray               # [9] (zeros without a model)
    best_iter: int
    iters: int
    max_good: int
    dk_capped: int              # hypotheses whose Durand-Kerner loop ran all DK_MAX_ITERS sweeps


def _hyp_points(h1, h2, subsets):
    return h1[subsets, 0], h1[subsets, 1], h2[subsets, 0], h2[subsets, 1]


def registrator_runs(sets, prob=0.999, max_iters=75):
    """RANSACPointSetRegistrator::run for many point sets [(h1, h2, thr)] at once -> [Run]."""
    hyps, owner = [], []
    subsets_of = {}
    for s, (h1, h2, thr) in enumerate(sets):
        m = len(h1)
        if m < MODEL_POINTS:
            continue
        if m == MODEL_POINTS:
            sub = np.arange(5, dtype=np.int32)[None]
        else:
            if m not in subsets_of:
                subsets_of[m] = rng_subsets(m, max_iters)
            sub = subsets_of[m]
        hyps.append(_hyp_points(h1, h2, sub))
        owner.append(s)
    runs = [None] * len(sets)
    if hyps:
        cat = [np.concatenate([h[k] for h in hyps]) for k in range(4)]
        E_all, V_all, sw_all = essential_kernel(*cat)
    off = 0
    for s, (h1, h2, thr) in enumerate(sets):
        r = Run()
        m = len(h1)
        r.mask, r.E, r.best_iter, r.iters, r.max_good, r.dk_capped = np.ones(m, np.uint8), np.zeros(9), -1, 0, 0, 0
        runs[s] = r
        if m < MODEL_POINTS:
            continue
        nh = 1 if m == MODEL_POINTS else max_iters
        E, V, sw = E_all[off:off + nh], V_all[off:off + nh], sw_all[off:off + nh]
        off += nh
        r.dk_capped = int((sw >= DK_MAX_ITERS).sum())
        if m == MODEL_POINTS:                                  # the single kernel call decides nothing but the model
            if V[0].any():
                r.E = E[0][np.argmax(V[0])].copy()
            continue
        t = np.float32(thr * thr)
        err = sampson_err(E, h1, h2)                           # [iters, 10, m]
        good = np.where(V, (err <= t).sum(axis=2), -1)
        niters, it, best, bk = max(max_iters, 1), 0, 0, None
        while it < niters:
            for k in range(10):
                g = int(good[it, k])
                if g >= 0 and g > max(best, MODEL_POINTS - 1):
                    best, bk = g, (it, k)
                    niters = update_num_iters(prob, (m - g) / m, MODEL_POINTS, niters)
            it += 1
        r.iters = it
        if best > 0:
            r.max_good, r.best_iter = best, bk[0]
            r.E = E[bk].copy()
            r.mask = (err[bk] <= t).astype(np.uint8)
    return runs


def do_ransac5(c1, c2, cam1, cam2, f1: float, f2: float, params: Params | None = None, run=None):
    """doRansac5 (ransac_pipeline.cpp:274-397, non-Theia) on the n tracked points -> (done, status [n] 0 / 3, E [9],
    summary [inliers, best iteration, iterations run, valid points], dk_capped). f* = (fx + fy) / 2 of each camera."""
    p = params or Params()
    n = len(c1)
    st = np.full(n, RANSAC_OUTLIER, np.int32)
    if n < MODEL_POINTS:
        return False, st, np.zeros(9), [0, -1, 0, 0], 0
    h1, h2, idx = normalize(c1, c2, cam1, cam2)
    if len(idx) < MODEL_POINTS:
        return False, st, np.zeros(9), [0, -1, 0, len(idx)], 0
    if run is None:
        run = registrator_runs([(h1, h2, threshold(f1, f2, p.ransac5Threshold))], p.ransac5Prob, p.ransacMaxIters)[0]
    st[idx[run.mask != 0]] = TRACKED
    return True, st, run.E, [int((st == TRACKED).sum()), run.best_iter, run.iters, len(idx)], run.dk_capped


def hybrid_select(n: int, r2_done: bool, r2_count: int, r5_done: bool, r5_count: int, use_r2: bool, params: Params | None = None):
    """computeHybridRansac's choice (ransac_pipeline.cpp:158-195) -> TYPE_SKIPPED / TYPE_R2 / TYPE_R5."""
    p = params or Params()
    f5 = r5_count / n if n else math.nan
    f2 = r2_count / n if n else math.nan
    if f5 < p.ransacMinInlierFraction:
        r5_done = False
    if f2 < p.ransacMinInlierFraction:
        r2_done = False
    if r2_done and not r5_done:
        return TYPE_R2
    if r5_done and not r2_done:
        return TYPE_R5
    if r2_done and r5_done:
        return TYPE_R2 if (use_r2 or r2_count > p.ransac2InliersOverRansac5Needed * r5_count) else TYPE_R5
    return TYPE_SKIPPED


def hybrid_pipeline(track_status, c1_all, c2_all, r2_status, r2_count: int, cam1, cam2, f1, f2, params: Params | None = None,
                    run=None):
    """RansacPipeline::compute on the hybrid path (ransac_pipeline.cpp:95-151) given RANSAC2's outcome on the TRACKED set.
    track_status [N] Feature::Status (TRACKED = 0), c*_all [N, 2], r2_status [N] (read at the TRACKED entries).
    -> (new track status [N], type, inlier count, stationarity score)."""
    p = params or Params()
    ts = np.array(track_status, np.int32).copy()
    sel = np.nonzero(ts == TRACKED)[0]
    n = len(sel)
    r2_done = n >= 2
    use_r2 = r2_count > p.ransac2InliersToSkipRansac5 * n
    r5_done, r5_count, st5 = False, 0, None
    if not use_r2:
        r5_done, st5, _, summ, _ = do_ransac5(np.asarray(c1_all)[sel], np.asarray(c2_all)[sel], cam1, cam2, f1, f2, p, run)
        r5_count = summ[0] if r5_done else 0
    typ = hybrid_select(n, r2_done, r2_count if r2_done else 0, r5_done, r5_count, use_r2, p)
    if typ == TYPE_SKIPPED:
        ts[:] = RANSAC_OUTLIER
        count = 0
    else:
        inl = (np.asarray(r2_status)[sel] == TRACKED) if typ == TYPE_R2 else (st5 == TRACKED)
        ts[sel[~inl]] = RANSAC_OUTLIER
        count = r2_count if typ == TYPE_R2 else r5_count
    score = r2_count / n if n else 0.0
    return ts, typ, count, score


# ---- synthetic two-view sets (test corpus) ----
def rotation(v):
    v = np.asarray(v, f64)
    th = float(np.linalg.norm(v))
    if th == 0:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def essential_truth(R, t):
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = (tx @ R).reshape(9)
    return E / np.linalg.norm(E)


def canonical(E):
    """Unit norm and the sign that makes the largest-magnitude entry positive."""
    E = np.asarray(E, f64) / np.linalg.norm(E)
    return E * np.sign(E[np.argmax(np.abs(E))])


CAMERAS = {
    "pinhole": ("pinhole", 400.0, 402.0, 376.0, 240.0, (), 180.0),
    "pinhole_radial": ("pinhole", 395.0, 398.0, 370.0, 236.0, (-0.25, 0.07, 0.0), 180.0),
    "fisheye": ("fisheye", 300.0, 301.0, 376.0, 240.0, (0.02, -0.01, 0.003, -0.0005), 170.0),
}


def make_set(rng, cam, n, outlier_frac, noise_px, scene="general", w=752, h=480):
    """One two-view set: cam = (orc.Camera, CAMERAS entry). Returns (c1 [n, 2] f32, c2 [n, 2] f32, inlier truth [n] bool,
    E truth [9]). Outliers lie >= 20 px (Sampson distance) off their epipolar line; noise is uniform in a disc of noise_px
    on the second view. Scene 'general': depths 2-6, baseline 0.5 (parallax that pins E down); 'planar' puts the points on
    one plane, 'rotation' makes the baseline 1e-4."""
    oc, spec = cam
    f = (spec[1] + spec[2]) * 0.5
    Rm = rotation(rng.normal(size=3) * 0.08)
    t = rng.normal(size=3)
    t *= (1e-4 if scene == "rotation" else 0.5) / np.linalg.norm(t)
    E = essential_truth(Rm, t)
    nrm_plane = rotation(rng.normal(size=3) * 0.3) @ np.array([0, 0, 1.0])
    c1, c2 = [], []
    while len(c1) < n:
        u, v = rng.uniform(20, w - 20), rng.uniform(20, h - 20)
        ok, ray = oc.pixel_to_ray(u, v)
        if not ok or ray[2] <= 0.2:
            continue
        if scene == "planar":                                        # plane n . X = 5
            d = 5.0 / float(nrm_plane @ ray)
            if d <= 0 or d > 50:
                continue
        else:
            d = rng.uniform(2.0, 6.0)
        X2 = Rm @ (ray * d) + t
        ok2, pix = oc.ray_to_pixel(X2)
        if not ok2 or not (0 <= pix[0] < w and 0 <= pix[1] < h):
            continue
        c1.append((u, v))
        c2.append(tuple(pix))
    c1, c2 = np.array(c1), np.array(c2)
    n_out = int(round(outlier_frac * n))
    truth = np.ones(n, bool)
    out_idx = rng.choice(n, n_out, replace=False) if n_out else np.zeros(0, np.int64)
    truth[out_idx] = False
    if noise_px > 0:
        ang, rad = rng.uniform(0, 2 * np.pi, n), noise_px * np.sqrt(rng.uniform(0, 1, n))
        c2 = c2 + np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    for i in out_idx:
        ok1, r1 = oc.pixel_to_ray(*c1[i])
        for _ in range(100):
            p = (rng.uniform(0, w), rng.uniform(0, h))
            ok2, r2 = oc.pixel_to_ray(*p)
            if not (ok2 and r2[2] > 0):
                continue
            a1, a2 = r1[:2] / r1[2], r2[:2] / r2[2]
            err = float(sampson_err(E[None], a1[None], a2[None])[0, 0])
            if math.sqrt(err) * f >= 20:
                c2[i] = p
                break
    return c1.astype(np.float32), c2.astype(np.float32), truth, E
