"""numpy restatement of the reference's stereo RANSAC3 track filter (doRansac3 and the tail of RansacPipeline::compute,
src/tracker/ransac_pipeline.cpp:95-151, 218-272) without Theia.

Test infrastructure only (imported by the tests, never by the product). It states the algorithm the device kernel
(hybvio_amd/csrc/ransac3.hip) runs, operation by operation in binary64; the kernel is built without FMA contraction, so
every elementwise numpy operation here rounds once, as the kernel does, and sums are written as explicit chains.

In the reference tree, followed to the letter:
  - the gather of doRansac3 (:224-251): TRACKED features in feature order, set to RANSAC_OUTLIER, Camera::normalizePixel
    (camera.cpp:471-476) of the previous-left, previous-right and current-left corner, triangulateStereoFeatureIdp
    (src/odometry/triangulation.cpp:711-764, (w)Mid2 with its c0 > min(c1, c2, c3) rejection), world_point =
    (idp.x, idp.y, 1) / idp.z, fewer than 3 correspondences = not run
  - the tail of compute (:121-123, 137-149).
  Within a three-term sum (dot products, squared norms, matrix times vector) the terms are added left to right; Eigen's
  own order inside such a sum is not pinned here (last bit only).

Recalled from Theia (not in the tree, therefore unpinned; DESIGN.md 3.14 lists the divergences):
  - SampleConsensusEstimator::Estimate with the RandomSampler: a persistent index vector 0..m-1, per iteration swapped
    at i = 0, 1, 2 with j = i + raw % (m - i), one raw std::mt19937 output per draw. `raw % range` is a deliberate
    departure from std::uniform_int_distribution, whose algorithm differs between libstdc++ versions and may reject draws.
  - ComputeMaxIterations with eps = DBL_EPSILON: ceil(logp / (log(1 - ratio^3) - eps)) clamped to
    [minIterations, maxIterations], ratio^3 written as (ratio * ratio) * ratio; max for ratio <= 0, min for ratio == 1.
  - The loop: models in iteration order, then solution order; a strictly lower cost replaces the best model; when the
    best model's inlier ratio is >= 3 / m the running limit becomes min(ComputeMaxIterations(3, ratio, logp), limit) (it
    only decreases); the loop ends when the iteration counter reaches the limit. The first limit is
    min(maxIterations, ComputeMaxIterations(3, ransacMinInlierFraction, logp)) (337 with the defaults).
  - The cost: useMle: sum of min-like terms (r < errorThresh ? r : errorThresh), added in correspondence order;
    otherwise m - inliers. Inlier: r < errorThresh; a non-finite residual is an outlier.
    r = |(R (X - c)).hnormalized() - feature|^2.

The minimal solver is NOT Theia's (Kneip-Scaramuzza-Siegwart): it is Grunert's P3P as in Haralick et al. (1994): the
quartic in v = s3 / s1, Ferrari's closed form for its real roots (largest real root of the resolvent cubic by Cardano /
the trigonometric form, two quadratics, three Newton steps per root on the monic quartic), u = s2 / s1 from v, two
Newton steps on the two distance-ratio equations in (u, v), the distances, and the rotation / position from the
orthonormal frames of the two triangles. Every real root gives a solution (up to 4, in root order); there is no cheirality
test. Solution order only decides ties. The solver takes the three correspondences of a sample in ascending index order,
whatever order the sampler listed them in: a triple that is drawn again then gives the same models and costs bit for bit,
ties with its first visit exactly and never replaces it (with three correspondences every iteration is such a repeat).
"""
from __future__ import annotations

import math

import numpy as np

f64 = np.float64
DBL_EPSILON = float(np.finfo(np.float64).eps)
DBL_MAX = float(np.finfo(np.float64).max)
TRACKED, RANSAC_OUTLIER = 0, 3
TYPE_SKIPPED, TYPE_R3 = 0, 2
CHUNK = 64                    # hypotheses solved per round (the kernel's chunk; the result does not depend on it)
MAX_ITERS = 500               # HV_RANSAC3_MAX_ITERS


class Params:
    """tracker.* parameters of RANSAC3 (codegen/parameter_definitions.c:282, 292-296)."""

    def __init__(self, ransac3ErrorThresh=1e-4, ransac3FailureProbability=1e-4, ransac3MaxIterations=500, ransac3MinIterations=50,
                 ransac3UseMle=1, ransacMinInlierFraction=0.3):
        self.ransac3ErrorThresh, self.ransac3FailureProbability = ransac3ErrorThresh, ransac3FailureProbability
        self.ransac3MaxIterations, self.ransac3MinIterations = ransac3MaxIterations, ransac3MinIterations
        self.ransac3UseMle, self.ransacMinInlierFraction = ransac3UseMle, ransacMinInlierFraction


def compute_max_iterations(k: int, ratio: float, logp: float, min_it: int, max_it: int) -> int:
    assert k == 3
    if ratio <= 0.0:
        return max_it
    if ratio == 1.0:
        return min_it
    lp = math.log(1.0 - (ratio * ratio) * ratio) - DBL_EPSILON
    v = math.ceil(logp / lp)
    return int(min(max(v, float(min_it)), float(max_it)))


def iteration_cap(p: Params) -> int:
    return min(p.ransac3MaxIterations, compute_max_iterations(3, p.ransacMinInlierFraction, math.log(p.ransac3FailureProbability),
                                                              p.ransac3MinIterations, p.ransac3MaxIterations))


# ---- the gather ----
def normalize_pixel(cam, x, y):
    """Camera::normalizePixel (camera.cpp:471-476) of a binary32 pixel -> (ok, u, v)."""
    ok, r = cam.pixel_to_ray(float(np.float32(x)), float(np.float32(y)))
    if not (ok and r[2] > 0):
        return False, 0.0, 0.0
    return True, r[0] / r[2], r[1] / r[2]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _matvec(M, v):
    return [_dot(M[i], v) for i in range(3)]


def triangulate_stereo_idp(ip_first, ip_second, T):
    """triangulateStereoFeatureIdp (triangulation.cpp:711-764) without the covariance, vectorised over points:
    ip_* [n, 2] normalised pixels, T = secondToFirstCamera (16 row-major doubles) -> (ok [n], idp [n, 3])."""
    ip_first, ip_second = np.asarray(ip_first, f64).reshape(-1, 2), np.asarray(ip_second, f64).reshape(-1, 2)
    T = np.asarray(T, f64).reshape(4, 4)
    one = np.ones(len(ip_first))
    f0 = [ip_second[:, 0], ip_second[:, 1], one]
    f1 = [ip_first[:, 0], ip_first[:, 1], one]
    with np.errstate(all="ignore"):
        n0, n1 = np.sqrt(_dot(f0, f0)), np.sqrt(_dot(f1, f1))
        f0h, f1h = [c / n0 for c in f0], [c / n1 for c in f1]
        R = [[T[i, j] for j in range(3)] for i in range(3)]
        t = [T[i, 3] * one for i in range(3)]
        Rf = _matvec(R, f0h)
        p, q, r = _cross(Rf, f1h), _cross(Rf, t), _cross(f1h, t)
        pn, qn, rn = np.sqrt(_dot(p, p)), np.sqrt(_dot(q, q)), np.sqrt(_dot(r, r))
        l0, l1 = rn / pn, qn / pn
        w = qn / (qn + rn)
        pf = [w * (t[i] + l0 * (Rf[i] + f1h[i])) for i in range(3)]
        a = _matvec([[l0 * R[i][j] for j in range(3)] for i in range(3)], f0h)       # lambda0 * R * f0hat
        b = [l1 * f1h[i] for i in range(3)]
        sq = lambda v: _dot(v, v)
        c0 = sq([(t[i] + a[i]) - b[i] for i in range(3)])
        c1 = sq([(t[i] + a[i]) + b[i] for i in range(3)])
        c2 = sq([(t[i] - a[i]) - b[i] for i in range(3)])
        c3 = sq([(t[i] - a[i]) + b[i] for i in range(3)])
        mn = np.where(c2 < c1, c2, c1)                                    # std::min(std::min(c1, c2), c3)
        mn = np.where(c3 < mn, c3, mn)
        ok = ~(c0 > mn)
        idp = np.stack([pf[0] / pf[2], pf[1] / pf[2], 1.0 / pf[2]], axis=1)
    return ok, idp


def gather(track_status, prev_left, prev_right, cur_left, cam0, cam1, T):
    """doRansac3 :224-251 -> (X [m, 3] world points, feat [m, 2], inds [m]); TRACKED = 0 entries only, feature order."""
    ts = np.asarray(track_status)
    cand, n00, n10, n01 = [], [], [], []
    for i in np.nonzero(ts == TRACKED)[0]:
        ok0, u0, v0 = normalize_pixel(cam0, *prev_left[i])
        ok1, u1, v1 = normalize_pixel(cam1, *prev_right[i])
        ok2, u2, v2 = normalize_pixel(cam0, *cur_left[i])
        if ok0 and ok1 and ok2:
            cand.append(i); n00.append((u0, v0)); n10.append((u1, v1)); n01.append((u2, v2))
    if not cand:
        return np.zeros((0, 3)), np.zeros((0, 2)), np.zeros(0, np.int64)
    ok, idp = triangulate_stereo_idp(np.array(n00), np.array(n10), T)
    with np.errstate(all="ignore"):
        X = np.stack([idp[:, 0] / idp[:, 2], idp[:, 1] / idp[:, 2], 1.0 / idp[:, 2]], axis=1)
    return X[ok], np.array(n01, f64)[ok], np.array(cand, np.int64)[ok]


# ---- the minimal solver ----
def quartic_real_roots(A4, A3, A2, A1, A0):
    """Real roots of A4 x^4 + ... + A0, vectorised: -> (x [H, 4], valid [H, 4]). Root order: the two roots of the first
    Ferrari quadratic (+ then -), then of the second."""
    with np.errstate(all="ignore"):
        a, b, c, d = A3 / A4, A2 / A4, A1 / A4, A0 / A4
        a2 = a * a
        p = b - 0.375 * a2
        q = (c - 0.5 * (a * b)) + 0.125 * (a2 * a)
        r = ((d - 0.25 * (a * c)) + 0.0625 * (a2 * b)) - 0.01171875 * (a2 * a2)
        # resolvent cubic m^3 + p m^2 + (p^2 / 4 - r) m - q^2 / 8 = 0, its largest real root
        k2, k1, k0 = p, 0.25 * (p * p) - r, -0.125 * (q * q)
        P = k1 - (k2 * k2) / 3.0
        Q = ((2.0 * ((k2 * k2) * k2)) / 27.0 - (k2 * k1) / 3.0) + k0
        D = 0.25 * (Q * Q) + ((P * P) * P) / 27.0
        sD = np.sqrt(np.where(D > 0, D, 0.0))
        t_one = np.cbrt(-0.5 * Q + sD) + np.cbrt(-0.5 * Q - sD)
        Pn = np.where(P < 0, P, -1.0)
        arg = ((3.0 * Q) / (2.0 * Pn)) * np.sqrt(-3.0 / Pn)
        arg = np.minimum(np.maximum(arg, -1.0), 1.0)
        t_three = (2.0 * np.sqrt(-Pn / 3.0)) * np.cos(np.arccos(arg) / 3.0)
        m = np.where(D > 0, t_one, t_three) - k2 / 3.0
        for _ in range(2):                                    # Newton on the cubic
            fm = ((m + k2) * m + k1) * m + k0
            dm = (3.0 * m + 2.0 * k2) * m + k1
            m = np.where(dm != 0, m - fm / np.where(dm != 0, dm, 1.0), m)
        ok = np.isfinite(m) & (m > 0) & (A4 != 0)
        s = np.sqrt(2.0 * np.where(ok, m, 1.0))
        h = 0.5 * p + m
        g = q / (2.0 * s)
        d1 = s * s - 4.0 * (h + g)
        d2 = s * s - 4.0 * (h - g)
        r1, r2 = np.sqrt(np.where(d1 >= 0, d1, 0.0)), np.sqrt(np.where(d2 >= 0, d2, 0.0))
        ys = [0.5 * (s + r1), 0.5 * (s - r1), 0.5 * (-s + r2), 0.5 * (-s - r2)]
        vs = [ok & (d1 >= 0), ok & (d1 >= 0), ok & (d2 >= 0), ok & (d2 >= 0)]
        xs = []
        for y in ys:
            x = y - 0.25 * a
            for _ in range(3):                                # Newton on the monic quartic
                fx = (((x + a) * x + b) * x + c) * x + d
                dx = ((4.0 * x + 3.0 * a) * x + 2.0 * b) * x + c
                x = np.where(dx != 0, x - fx / np.where(dx != 0, dx, 1.0), x)
            xs.append(x)
    return np.stack(xs, axis=1), np.stack(vs, axis=1)


def _frame(A, B, C):
    """Orthonormal frame of the triangle A, B, C: e1 along AB, e3 normal, e2 = e3 x e1."""
    d1 = [B[i] - A[i] for i in range(3)]
    d2 = [C[i] - A[i] for i in range(3)]
    n1 = np.sqrt(_dot(d1, d1))
    e1 = [c / n1 for c in d1]
    w = _cross(e1, d2)
    n3 = np.sqrt(_dot(w, w))
    e3 = [c / n3 for c in w]
    return e1, _cross(e3, e1), e3


def p3p(X, feat):
    """X [H, 3, 3] world points, feat [H, 3, 2] normalised image points -> (R [H, 4, 9] row-major, c [H, 4, 3],
    valid [H, 4]) with x_cam = R (X - c)."""
    X, feat = np.asarray(X, f64), np.asarray(feat, f64)
    H = X.shape[0]
    Rm, cm, valid = np.zeros((H, 4, 9)), np.zeros((H, 4, 3)), np.zeros((H, 4), bool)
    if H == 0:
        return Rm, cm, valid
    with np.errstate(all="ignore"):
        P = [[X[:, k, i] for i in range(3)] for k in range(3)]
        j = []
        for k in range(3):
            u, v = feat[:, k, 0], feat[:, k, 1]
            n = np.sqrt((u * u + v * v) + 1.0)
            j.append([u / n, v / n, 1.0 / n])
        d2 = lambda A, B: _dot([A[i] - B[i] for i in range(3)], [A[i] - B[i] for i in range(3)])
        a2, b2, c2 = d2(P[1], P[2]), d2(P[0], P[2]), d2(P[0], P[1])
        ca, cb, cg = _dot(j[1], j[2]), _dot(j[0], j[2]), _dot(j[0], j[1])
        q1, q2, q3, q4, ra, rc = (a2 - c2) / b2, (a2 + c2) / b2, (b2 - c2) / b2, (b2 - a2) / b2, a2 / b2, c2 / b2
        ca2, cb2, cg2 = ca * ca, cb * cb, cg * cg
        A4 = (q1 - 1.0) * (q1 - 1.0) - (4.0 * rc) * ca2
        A3 = 4.0 * (((q1 * (1.0 - q1)) * cb - ((1.0 - q2) * ca) * cg) + ((2.0 * rc) * ca2) * cb)
        A2 = 2.0 * ((((((q1 * q1 - 1.0) + ((2.0 * (q1 * q1)) * cb2)) + (2.0 * q3) * ca2) - (((4.0 * q2) * ca) * cb) * cg)
                     + (2.0 * q4) * cg2))
        A1 = 4.0 * (((-(q1 * (1.0 + q1))) * cb + ((2.0 * ra) * cg2) * cb) - ((1.0 - q2) * ca) * cg)
        A0 = (1.0 + q1) * (1.0 + q1) - (4.0 * ra) * cg2
        roots, rvalid = quartic_real_roots(A4, A3, A2, A1, A0)
        for s in range(4):
            v = roots[:, s]
            u = ((((q1 - 1.0) * (v * v) - ((2.0 * q1) * cb) * v) + 1.0) + q1) / (2.0 * (cg - v * ca))
            for _ in range(2):                                # Newton on the two distance-ratio equations in (u, v)
                w = (1.0 + v * v) - (2.0 * v) * cb
                f1 = ((1.0 + u * u) - (2.0 * u) * cg) - w * rc
                f2 = ((u * u + v * v) - ((2.0 * u) * v) * ca) - w * ra
                j11, j12 = 2.0 * (u - cg), (-2.0 * (v - cb)) * rc
                j21, j22 = 2.0 * (u - v * ca), 2.0 * (v - u * ca) - (2.0 * (v - cb)) * ra
                det = j11 * j22 - j12 * j21
                good = np.isfinite(det) & (det != 0)
                dets = np.where(good, det, 1.0)
                u = np.where(good, u - (j22 * f1 - j12 * f2) / dets, u)
                v = np.where(good, v - (j11 * f2 - j21 * f1) / dets, v)
            s1 = np.sqrt(b2 / ((1.0 + v * v) - (2.0 * v) * cb))
            s2, s3 = u * s1, v * s1
            Y = [[s1 * j[0][i] for i in range(3)], [s2 * j[1][i] for i in range(3)], [s3 * j[2][i] for i in range(3)]]
            e = _frame(P[0], P[1], P[2])
            g = _frame(Y[0], Y[1], Y[2])
            R = [[(g[0][i] * e[0][k] + g[1][i] * e[1][k]) + g[2][i] * e[2][k] for k in range(3)] for i in range(3)]
            # c = X1 - R^T Y1
            c = [P[0][k] - ((R[0][k] * Y[0][0] + R[1][k] * Y[0][1]) + R[2][k] * Y[0][2]) for k in range(3)]
            fin = rvalid[:, s].copy()
            for i in range(3):
                for k in range(3):
                    Rm[:, s, 3 * i + k] = R[i][k]
                    fin &= np.isfinite(R[i][k])
                cm[:, s, i] = c[i]
                fin &= np.isfinite(c[i])
            valid[:, s] = fin
    return Rm, cm, valid


def residuals(R, c, X, feat):
    """R [..., 9], c [..., 3] against X [m, 3], feat [m, 2] -> [..., m] squared reprojection errors."""
    with np.errstate(all="ignore"):
        d = [X[:, k] - c[..., k, None] for k in range(3)]
        p = [(R[..., 3 * i, None] * d[0] + R[..., 3 * i + 1, None] * d[1]) + R[..., 3 * i + 2, None] * d[2] for i in range(3)]
        e0, e1 = p[0] / p[2] - feat[:, 0], p[1] / p[2] - feat[:, 1]
        return e0 * e0 + e1 * e1


# ---- the sampler and the loop ----
class Sampler:
    """Theia's RandomSampler as recalled: a persistent index vector, partially shuffled per sample."""

    def __init__(self, m: int, draws):
        self.idx, self.draws, self.pos, self.m = list(range(m)), np.asarray(draws, np.uint32), 0, m

    def sample(self):
        for i in range(3):
            j = i + int(self.draws[self.pos]) % (self.m - i)
            self.pos += 1
            self.idx[i], self.idx[j] = self.idx[j], self.idx[i]
        return self.idx[0], self.idx[1], self.idx[2]


class Run:
    mask: np.ndarray            # [m] bool, the best model's inliers
    pose: np.ndarray            # [12] R row-major, then the position; zeros without a model
    best_iter: int
    iters: int
    success: bool


def ransac(X, feat, draws, params: Params | None = None) -> Run:
    """EstimateCalibratedAbsolutePose with RansacType::RANSAC on m >= 3 correspondences; draws = the next
    3 * ransac3MaxIterations raw outputs of the generator (3 * Run.iters of them are consumed)."""
    p = params or Params()
    m = len(X)
    assert m >= 3
    thr = p.ransac3ErrorThresh
    logp = math.log(p.ransac3FailureProbability)
    cap = iteration_cap(p)
    sampler = Sampler(m, draws)
    limit, it, best_cost = cap, 0, DBL_MAX
    r = Run()
    r.mask, r.pose, r.best_iter, r.success = np.zeros(m, bool), np.zeros(12), -1, False
    while it < limit:
        h = min(CHUNK, cap - it)
        tri = np.sort(np.array([sampler.sample() for _ in range(h)], np.int64), axis=1)   # the solver's canonical order
        Rm, cm, valid = p3p(X[tri], feat[tri])
        res = residuals(Rm, cm, X, feat)                                   # [h, 4, m]
        inl = res < thr
        count = inl.sum(axis=2)
        if p.ransac3UseMle:
            cost = np.cumsum(np.where(inl, res, thr), axis=2)[:, :, -1]   # cumsum adds left to right
        else:
            cost = (m - count).astype(f64)
        for k in range(h):
            if it >= limit:
                break
            for s in range(4):
                if valid[k, s] and cost[k, s] < best_cost:
                    best_cost = float(cost[k, s])
                    r.success, r.best_iter, r.mask = True, it, inl[k, s].copy()
                    r.pose = np.concatenate([Rm[k, s], cm[k, s]])
                    ratio = int(count[k, s]) / m
                    if not ratio < 3.0 / m:
                        limit = min(compute_max_iterations(3, ratio, logp, p.ransac3MinIterations, p.ransac3MaxIterations), limit)
            it += 1
    r.iters = it
    return r


def do_ransac3(track_status, prev_left, prev_right, cur_left, cam0, cam1, T, draws, params: Params | None = None):
    """doRansac3 (:218-272) -> (new status [n], done, inlier count, pose [12], summary [inliers, best iteration, iterations
    run, correspondences])."""
    ts = np.array(track_status, np.int32).copy()
    X, feat, inds = gather(ts, prev_left, prev_right, cur_left, cam0, cam1, T)
    ts[ts == TRACKED] = RANSAC_OUTLIER
    m = len(inds)
    if m < 3:
        return ts, False, 0, np.zeros(12), [0, -1, 0, m]
    run = ransac(X, feat, draws, params)
    if not run.success:
        return ts, False, 0, np.zeros(12), [0, -1, run.iters, m]
    ts[inds[run.mask]] = TRACKED
    cnt = int(run.mask.sum())
    return ts, True, cnt, run.pose, [cnt, run.best_iter, run.iters, m]


def compute(track_status, prev_left, prev_right, cur_left, cam0, cam1, T, draws, r2_count: int, params: Params | None = None):
    """RansacPipeline::compute on the RANSAC3 branch given RANSAC2's bestInlierCount on the TRACKED set
    -> (new status [n], type, inlierCount, score, summary)."""
    n_tracked = int((np.asarray(track_status) == TRACKED).sum())
    ts, done, cnt, _, summ = do_ransac3(track_status, prev_left, prev_right, cur_left, cam0, cam1, T, draws, params)
    if not done:
        ts[:] = RANSAC_OUTLIER                                             # :139-144
    score = (r2_count if n_tracked >= 2 else 0) / n_tracked if n_tracked else 0.0
    return ts, (TYPE_R3 if done else TYPE_SKIPPED), cnt, score, summ


# ---- synthetic stereo sets (test corpus) ----
def rotation(v):
    v = np.asarray(v, f64)
    th = float(np.linalg.norm(v))
    if th == 0:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


BASELINE = 0.11
SECOND_TO_FIRST = np.array([1, 0, 0, BASELINE, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1], f64)   # X_first = X_second + (b, 0, 0)


def make_set(rng, cam, n, outlier_frac, noise_px, n_untracked=0, n_diverging=0, n_outside=0, w=752, h=480):
    """One stereo set for a rig of two equal cameras (cam = orc.Camera), the second one BASELINE to the right: n good
    features (depths 1.5-8, motion ~ N(0, 0.02) rad, N(0, 0.05) translation) of which round(outlier_frac n) have their
    current corner moved 20-60 px; noise uniform in a disc of noise_px on all three corners. Interleaved with them:
    n_untracked entries with a non-TRACKED status, n_diverging whose right corner lies on the wrong side (the rays diverge,
    the triangulation is rejected) and n_outside whose current corner lies outside a fisheye's valid field of view (far
    outside the image). -> dict(status, prev_left, prev_right, cur_left [N, 2] f32, truth [N] bool (inlier expected),
    pose_true [12])."""
    Rm = rotation(rng.normal(size=3) * 0.02)
    c = rng.normal(size=3) * 0.05
    pl, pr, cl = [], [], []
    while len(pl) < n + n_diverging + n_outside:
        u, v = rng.uniform(20, w - 20), rng.uniform(20, h - 20)
        ok, ray = cam.pixel_to_ray(u, v)
        if not ok or ray[2] <= 0.2:
            continue
        X = ray / ray[2] * rng.uniform(1.5, 8.0)
        ok1, p1 = cam.ray_to_pixel(X - np.array([BASELINE, 0, 0]))
        ok2, p2 = cam.ray_to_pixel(Rm @ (X - c))
        if not (ok1 and ok2 and 0 <= p1[0] < w and 0 <= p1[1] < h and 0 <= p2[0] < w and 0 <= p2[1] < h):
            continue
        pl.append((u, v)); pr.append(tuple(p1)); cl.append(tuple(p2))
    pl, pr, cl = np.array(pl).reshape(-1, 2), np.array(pr).reshape(-1, 2), np.array(cl).reshape(-1, 2)
    if noise_px > 0:
        for a in (pl, pr, cl):
            ang, rad = rng.uniform(0, 2 * np.pi, len(a)), noise_px * np.sqrt(rng.uniform(0, 1, len(a)))
            a += np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    truth = np.ones(len(pl), bool)
    n_out = int(round(outlier_frac * n))
    out_idx = rng.choice(n, n_out, replace=False) if n_out else np.zeros(0, np.int64)
    ang, rad = rng.uniform(0, 2 * np.pi, n_out), rng.uniform(20, 60, n_out)
    cl[out_idx] += np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    truth[out_idx] = False
    for i in range(n, n + n_diverging):                                   # disparity of the wrong sign, 15-30 px
        pr[i, 0] = pl[i, 0] + rng.uniform(15, 30)
        truth[i] = False
    for i in range(n + n_diverging, n + n_diverging + n_outside):
        cl[i] = (-150.0 - rng.uniform(0, 50), -120.0 - rng.uniform(0, 50))
        truth[i] = False
    N = len(pl) + n_untracked
    order = rng.permutation(N)
    status = np.zeros(N, np.int32)
    P = [np.zeros((N, 2)), np.zeros((N, 2)), np.zeros((N, 2))]
    tr = np.zeros(N, bool)
    for dst, src in enumerate(order):
        if src < len(pl):
            P[0][dst], P[1][dst], P[2][dst], tr[dst] = pl[src], pr[src], cl[src], truth[src]
        else:
            status[dst] = int(rng.choice([2, 4, 6]))
            for a in P:
                a[dst] = (rng.uniform(0, w), rng.uniform(0, h))
    return dict(status=status, prev_left=P[0].astype(np.float32), prev_right=P[1].astype(np.float32),
                cur_left=P[2].astype(np.float32), truth=tr, pose_true=np.concatenate([Rm.reshape(9), c]))
