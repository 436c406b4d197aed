"""numpy restatement of the reference's stereo upright 2-point track filter (StereoUpright2p::compute,
src/tracker/stereo_upright_2p.cpp, and the UPRIGHT_2P branch and tail of RansacPipeline::compute,
src/tracker/ransac_pipeline.cpp:124-127, 137-149) without Theia.

Test infrastructure only (imported by the tests, never by the product). It states the algorithm the device kernel
(hybvio_amd/csrc/upright2p.hip) runs, operation by operation in binary64; the kernel is built without FMA contraction, so
every elementwise numpy operation here rounds once, as the kernel does, and sums are written as explicit chains.

In the reference tree, followed to the letter:
  - the gather (stereo_upright_2p.cpp:118-163): TRACKED features in feature order, set to RANSAC_OUTLIER,
    Camera::normalizePixel of the previous-left (camera0) and previous-right (camera1) corner,
    triangulateStereoFeatureIdp with secondToFirstCamera, model point (idp.x, idp.y, 1) / idp.z (these three are imported
    from ransac3_restatement), Camera::pixelToRay of the current-left corner (camera0; no test of the ray's depth), the
    correspondence modelPoint = R0 X, ray = R1 ray_cam, rayNormalized = ray_cam.xy / ray_cam.z with R0, R1 the top-left 3x3
    of poses[0], poses[1]; fewer than 2 correspondences = not run
  - the error (:72-81): w = R modelPoint + t, p = worldToCamera w, |p.xy / p.z - rayNormalized|^2. The reference's
    worldToCamera is R1.inverse(); here it is the transpose of R1 (a departure of last bits: R1 is a rotation).
  - the tail of compute (:124-127, 137-149).
  Within a three-term sum the terms are added left to right, as in ransac3_restatement.

Recalled from Theia (not in the tree; the same recollection as ransac3_restatement, with a sample of 2):
  - the RandomSampler: a persistent index vector 0..m-1, per iteration swapped at i = 0, 1 with j = i + raw % (m - i), one
    raw std::mt19937 output per draw
  - ComputeMaxIterations: ceil(logp / (log(1 - ratio * ratio) - eps)) clamped to [min, max]; max for ratio <= 0, min for
    ratio == 1. The first limit is min(maxIterations, ComputeMaxIterations(2, ransacMinInlierFraction, logp)), 98 with the
    defaults.
  - the loop: models in iteration order, then root order; a strictly lower cost replaces the best model; when the best
    model's inlier ratio is >= 2 / m the limit becomes min(ComputeMaxIterations(2, ratio, logp), limit)
  - the cost: useMle: sum of (r < thresh ? r : thresh) in correspondence order; otherwise m - inliers. A non-finite
    residual is an outlier.

The minimal solver is NOT Theia's TwoPointPosePartialRotation; it is stated here. It finds the rotation R = Rz(theta) about
(0, 0, 1) and the translation t with R X_i + t = lambda_i r_i, i = 0, 1:
  the point whose ray has the larger |r.z| is index 1 (the pair is swapped otherwise; t comes out the same);
  D = X0 - X1, n2 = Dx^2 + Dy^2; the z row gives lambda1 = k lambda0 - D.z / r1.z with k = r0.z / r1.z; the x, y rows give
  R D.xy = lambda0 b + a with b = r0.xy - k r1.xy, a = (D.z / r1.z) r1.xy; a rotation keeps the length:
  |b|^2 lambda0^2 + 2 (a.b) lambda0 + (|a|^2 - n2) = 0. Its roots in ascending order of the formula, (-B - sqrt(disc)) / A then
  (-B + sqrt(disc)) / A with A = |b|^2, B = a.b, C = |a|^2 - n2, disc = B^2 - A C, each give d = lambda0 b + a,
  c = Dx d.x + Dy d.y, s = Dx d.y - Dy d.x, both divided by hypot(c, s) written as sqrt(c c + s s) (one correctly rounded
  operation per step on the host and on the device), R = [[c, -s, 0], [s, c, 0], [0, 0, 1]], t = lambda0 r0 - R X0.
  No solution when n2 == 0, r1.z == 0, A == 0, disc < 0 or anything is non-finite. There is no cheirality test (lambda may
  be negative), as for P3P: the reference's error metric is sign-blind as well. The sample is handed to the solver in
  ascending index order, so a pair that is drawn again ties with its first visit exactly.
"""
from __future__ import annotations

import math

import numpy as np

import ransac3_restatement as R3
from ransac3_restatement import normalize_pixel, triangulate_stereo_idp, rotation, SECOND_TO_FIRST, BASELINE  # noqa: F401

f64 = np.float64
DBL_EPSILON = R3.DBL_EPSILON
DBL_MAX = R3.DBL_MAX
TRACKED, RANSAC_OUTLIER = 0, 3
TYPE_SKIPPED, TYPE_UPRIGHT_2P = 0, 4
CHUNK = 128                   # hypotheses per round (the kernel's chunk; the result does not depend on it)
MAX_ITERS = 500               # HV_UPRIGHT2P_MAX_ITERS
SAMPLE = 2


class Params:
    """tracker.* parameters of the filter (codegen/parameter_definitions.c:282, 299-303)."""

    def __init__(self, ransacStereoUpright2pErrorThresh=1e-4, ransacStereoUpright2pFailureProbability=1e-4,
                 ransacStereoUpright2pMaxIterations=500, ransacStereoUpright2pMinIterations=50, ransacStereoUpright2pUseMle=1,
                 ransacMinInlierFraction=0.3):
        self.ransacStereoUpright2pErrorThresh = ransacStereoUpright2pErrorThresh
        self.ransacStereoUpright2pFailureProbability = ransacStereoUpright2pFailureProbability
        self.ransacStereoUpright2pMaxIterations = ransacStereoUpright2pMaxIterations
        self.ransacStereoUpright2pMinIterations = ransacStereoUpright2pMinIterations
        self.ransacStereoUpright2pUseMle = ransacStereoUpright2pUseMle
        self.ransacMinInlierFraction = ransacMinInlierFraction


def compute_max_iterations(k: int, ratio: float, logp: float, min_it: int, max_it: int) -> int:
    """ransac3_restatement.compute_max_iterations by the sample size: ratio^k written as a left-to-right product."""
    assert k in (2, 3)
    if ratio <= 0.0:
        return max_it
    if ratio == 1.0:
        return min_it
    pw = ratio * ratio
    if k == 3:
        pw = pw * ratio
    lp = math.log(1.0 - pw) - DBL_EPSILON
    v = math.ceil(logp / lp)
    return int(min(max(v, float(min_it)), float(max_it)))


def iteration_cap(p: Params) -> int:
    return min(p.ransacStereoUpright2pMaxIterations,
               compute_max_iterations(SAMPLE, p.ransacMinInlierFraction, math.log(p.ransacStereoUpright2pFailureProbability),
                                      p.ransacStereoUpright2pMinIterations, p.ransacStereoUpright2pMaxIterations))


def rot3(poses):
    """The top-left 3x3 of poses[0] and poses[1] (two row-major 4x4) -> (R0, R1) as [3][3]."""
    P = np.asarray(poses, f64).reshape(2, 4, 4)
    return P[0, :3, :3].copy(), P[1, :3, :3].copy()


def _rot(R, v):
    """R v for v = list of three arrays, every row a left-to-right chain."""
    return [(R[i][0] * v[0] + R[i][1] * v[1]) + R[i][2] * v[2] for i in range(3)]


# ---- the gather ----
def gather(track_status, prev_left, prev_right, cur_left, cam0, cam1, T, poses, perturb=None):
    """stereo_upright_2p.cpp:124-160 -> (X [m, 3] rotated model points, ray [m, 3] rotated rays, rn [m, 2], inds [m]).
    perturb(a) (tests only) maps every array of normalised coordinates / ray components before they are used."""
    ts = np.asarray(track_status)
    R0, R1 = rot3(poses)
    pt = perturb or (lambda a: a)
    cand, n00, n10, rays = [], [], [], []
    for i in np.nonzero(ts == TRACKED)[0]:
        ok0, u0, v0 = normalize_pixel(cam0, *prev_left[i])
        ok1, u1, v1 = normalize_pixel(cam1, *prev_right[i])
        if not (ok0 and ok1):
            continue
        cand.append(i); n00.append((u0, v0)); n10.append((u1, v1))
    empty = (np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 2)), np.zeros(0, np.int64))
    if not cand:
        return empty
    ok, idp = triangulate_stereo_idp(pt(np.array(n00, f64)), pt(np.array(n10, f64)), T)
    keep = []
    for q, i in enumerate(cand):
        if not ok[q]:
            continue
        okr, r = cam0.pixel_to_ray(float(np.float32(cur_left[i][0])), float(np.float32(cur_left[i][1])))
        if not okr:
            continue
        keep.append(q); rays.append((r[0], r[1], r[2]))
    if not keep:
        return empty
    idp = idp[keep]
    rc = pt(np.array(rays, f64))
    with np.errstate(all="ignore"):
        Xc = [idp[:, 0] / idp[:, 2], idp[:, 1] / idp[:, 2], 1.0 / idp[:, 2]]
        X = np.stack(_rot(R0, Xc), axis=1)
        ray = np.stack(_rot(R1, [rc[:, 0], rc[:, 1], rc[:, 2]]), axis=1)
        rn = np.stack([rc[:, 0] / rc[:, 2], rc[:, 1] / rc[:, 2]], axis=1)
    return X, ray, rn, np.array(cand, np.int64)[keep]


# ---- the minimal solver ----
def solve(X, r):
    """X [H, 2, 3] model points, r [H, 2, 3] rays -> (model [H, 2, 5] = (c, s, tx, ty, tz), valid [H, 2]): the rotation
    [[c, -s, 0], [s, c, 0], [0, 0, 1]] and the translation, per root."""
    X, r = np.asarray(X, f64), np.asarray(r, f64)
    H = X.shape[0]
    model, valid = np.zeros((H, 2, 5)), np.zeros((H, 2), bool)
    if H == 0:
        return model, valid
    with np.errstate(all="ignore"):
        swap = np.abs(r[:, 0, 2]) > np.abs(r[:, 1, 2])                     # index 1 has the larger |r.z|
        sel = lambda A, k: [np.where(swap, A[:, 1 - k, i], A[:, k, i]) for i in range(3)]
        X0, X1, r0, r1 = sel(X, 0), sel(X, 1), sel(r, 0), sel(r, 1)
        D = [X0[i] - X1[i] for i in range(3)]
        n2 = D[0] * D[0] + D[1] * D[1]
        k = r0[2] / r1[2]
        b = [r0[0] - k * r1[0], r0[1] - k * r1[1]]
        q = D[2] / r1[2]
        a = [q * r1[0], q * r1[1]]
        A = b[0] * b[0] + b[1] * b[1]
        B = a[0] * b[0] + a[1] * b[1]
        C = (a[0] * a[0] + a[1] * a[1]) - n2
        disc = B * B - A * C
        base = (n2 != 0) & (r1[2] != 0) & (A != 0) & (disc >= 0)
        sq = np.sqrt(np.where(disc >= 0, disc, 0.0))
        for root, l0 in enumerate(((-B - sq) / A, (-B + sq) / A)):
            d = [l0 * b[0] + a[0], l0 * b[1] + a[1]]
            c = D[0] * d[0] + D[1] * d[1]
            s = D[0] * d[1] - D[1] * d[0]
            h = np.sqrt(c * c + s * s)
            c, s = c / h, s / h
            t = [l0 * r0[0] - (c * X0[0] - s * X0[1]), l0 * r0[1] - (s * X0[0] + c * X0[1]), l0 * r0[2] - X0[2]]
            fin = base.copy()
            for j, v in enumerate((c, s, t[0], t[1], t[2])):
                model[:, root, j] = v
                fin &= np.isfinite(v)
            valid[:, root] = fin
    return model, valid


def model12(mod):
    """(c, s, tx, ty, tz) -> [12]: R row-major, then t."""
    c, s, tx, ty, tz = (float(v) for v in mod)
    return np.array([c, -s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0, tx, ty, tz])


def residuals(mod, X, rn, R1):
    """mod [..., 5] against X [m, 3], rn [m, 2] -> [..., m] squared errors (stereo_upright_2p.cpp:72-81, R1 transposed)."""
    with np.errstate(all="ignore"):
        c, s = mod[..., 0, None], mod[..., 1, None]
        w = [(c * X[:, 0] - s * X[:, 1]) + mod[..., 2, None], (s * X[:, 0] + c * X[:, 1]) + mod[..., 3, None], X[:, 2] + mod[..., 4, None]]
        p = [(R1[0][i] * w[0] + R1[1][i] * w[1]) + R1[2][i] * w[2] for i in range(3)]
        e0, e1 = p[0] / p[2] - rn[:, 0], p[1] / p[2] - rn[:, 1]
        return e0 * e0 + e1 * e1


# ---- the sampler and the loop ----
class Sampler:
    """ransac3_restatement.Sampler by the sample size."""

    def __init__(self, m: int, draws, k: int = SAMPLE):
        self.idx, self.draws, self.pos, self.m, self.k = list(range(m)), np.asarray(draws, np.uint32), 0, m, k

    def sample(self):
        for i in range(self.k):
            j = i + int(self.draws[self.pos]) % (self.m - i)
            self.pos += 1
            self.idx[i], self.idx[j] = self.idx[j], self.idx[i]
        return tuple(self.idx[:self.k])


class Run:
    mask: np.ndarray            # [m] bool, the best model's inliers
    model: np.ndarray           # [12] R row-major, then t; zeros without a model
    best_iter: int
    iters: int
    success: bool


def ransac(X, ray, rn, R1, draws, params: Params | None = None) -> Run:
    """The sample-consensus loop on m >= 2 correspondences; draws = the next 2 * MaxIterations raw outputs of the
    generator (2 * Run.iters of them are consumed)."""
    p = params or Params()
    m = len(X)
    assert m >= SAMPLE
    thr = p.ransacStereoUpright2pErrorThresh
    logp = math.log(p.ransacStereoUpright2pFailureProbability)
    mn, mx = p.ransacStereoUpright2pMinIterations, p.ransacStereoUpright2pMaxIterations
    cap = iteration_cap(p)
    sampler = Sampler(m, draws)
    limit, it, best_cost = cap, 0, DBL_MAX
    r = Run()
    r.mask, r.model, r.best_iter, r.success = np.zeros(m, bool), np.zeros(12), -1, False
    while it < limit:
        h = min(CHUNK, cap - it)
        pair = np.sort(np.array([sampler.sample() for _ in range(h)], np.int64), axis=1)   # the solver's canonical order
        mod, valid = solve(X[pair], ray[pair])
        res = residuals(mod, X, rn, R1)                                     # [h, 2, m]
        inl = res < thr
        count = inl.sum(axis=2)
        if p.ransacStereoUpright2pUseMle:
            cost = np.cumsum(np.where(inl, res, thr), axis=2)[:, :, -1]   # cumsum adds left to right
        else:
            cost = (m - count).astype(f64)
        for k in range(h):
            if it >= limit:
                break
            for s in range(2):
                if valid[k, s] and cost[k, s] < best_cost:
                    best_cost = float(cost[k, s])
                    r.success, r.best_iter, r.mask = True, it, inl[k, s].copy()
                    r.model = model12(mod[k, s])
                    ratio = int(count[k, s]) / m
                    if not ratio < 2.0 / m:
                        limit = min(compute_max_iterations(SAMPLE, ratio, logp, mn, mx), limit)
            it += 1
    r.iters = it
    return r


def do_upright2p(track_status, prev_left, prev_right, cur_left, cam0, cam1, T, poses, draws, params: Params | None = None, perturb=None):
    """StereoUpright2p::compute -> (new status [n], done, inlier count, model [12], summary [inliers, best iteration,
    iterations run, correspondences])."""
    ts = np.array(track_status, np.int32).copy()
    X, ray, rn, inds = gather(ts, prev_left, prev_right, cur_left, cam0, cam1, T, poses, perturb)
    ts[ts == TRACKED] = RANSAC_OUTLIER
    m = len(inds)
    if m < SAMPLE:
        return ts, False, 0, np.zeros(12), [0, -1, 0, m]
    run = ransac(X, ray, rn, rot3(poses)[1], draws, params)
    if not run.success:
        return ts, False, 0, np.zeros(12), [0, -1, run.iters, m]
    ts[inds[run.mask]] = TRACKED
    cnt = int(run.mask.sum())
    return ts, True, cnt, run.model, [cnt, run.best_iter, run.iters, m]


def compute(track_status, prev_left, prev_right, cur_left, cam0, cam1, T, poses, draws, r2_count: int, params: Params | None = None):
    """RansacPipeline::compute on the upright branch given RANSAC2's bestInlierCount on the TRACKED set
    -> (new status [n], type, inlierCount, score, summary)."""
    n_tracked = int((np.asarray(track_status) == TRACKED).sum())
    ts, done, cnt, _, summ = do_upright2p(track_status, prev_left, prev_right, cur_left, cam0, cam1, T, poses, draws, params)
    if not done:
        ts[:] = RANSAC_OUTLIER                                             # :139-144
    score = (r2_count if n_tracked >= 2 else 0) / n_tracked if n_tracked else 0.0
    return ts, (TYPE_UPRIGHT_2P if done else TYPE_SKIPPED), cnt, score, summ


# ---- synthetic stereo sets (test corpus) ----
def rz(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


ATTITUDES = ("general", "up", "down", "horizontal")


def attitude(rng, kind):
    """A camera-to-world rotation: 'general' = any; 'up' / 'down' = the optical axis within ~3 degrees of the world's
    +z / -z; 'horizontal' = the optical axis within ~3 degrees of the horizon."""
    if kind == "general":
        return rotation(rng.normal(size=3) * 1.5)
    small = rotation(rng.normal(size=3) * 0.03)
    yaw = rz(rng.uniform(-math.pi, math.pi))
    if kind == "up":
        base = np.eye(3)
    elif kind == "down":
        base = np.diag([1.0, -1.0, -1.0])
    else:
        base = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])     # camera z -> world y, camera y -> world -z
    return yaw @ small @ base


def make_set(rng, cam, n, outlier_frac, noise_px, n_untracked=0, n_diverging=0, n_outside=0, kind="general", psi=0.0, tilt_deg=0.0,
             w=752, h=480):
    """ransac3_restatement.make_set (the rig, the points, the noise, the outliers and the interleaved special entries) with
    the filter's poses: R0 = attitude(kind) is the previous camera-to-world rotation; the generator's motion x1 = Rm (X - c)
    makes the true current one R1_true = R0 Rm^T; the filter is handed R1_est = Rz(psi) Rtilt(eps) R1_true, a yaw error that
    the model absorbs and a roll / pitch error of tilt_deg about a random horizontal axis that it does not. Adds poses [32]
    (positions arbitrary: the filter reads the rotations only) and model_true [12] = (Rz(psi), -Rz(psi) R0 c), exact for
    tilt_deg == 0."""
    d = R3.make_set(rng, cam, n, outlier_frac, noise_px, n_untracked, n_diverging, n_outside, w, h)
    Rm, c = d["pose_true"][:9].reshape(3, 3), d["pose_true"][9:]
    R0 = attitude(rng, kind)
    ax = rng.uniform(0, 2 * math.pi)
    tilt = rotation(np.array([math.cos(ax), math.sin(ax), 0.0]) * math.radians(tilt_deg))
    R1 = rz(psi) @ tilt @ (R0 @ Rm.T)
    P = np.zeros((2, 4, 4))
    P[0, :3, :3], P[1, :3, :3] = R0, R1
    P[0, :3, 3], P[1, :3, 3] = rng.normal(size=3), rng.normal(size=3)
    P[:, 3, 3] = 1.0
    d["poses"] = P.reshape(32)
    d["model_true"] = np.concatenate([rz(psi).reshape(9), -(rz(psi) @ (R0 @ c))])
    return d
