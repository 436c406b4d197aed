"""GPU tests of the EKF control entries (hv_ekf_block_update_dev, hv_ekf_pseudo_velocity_dev, hv_ekf_undo_augment_dev,
hv_ekf_imu_control_dev, hv_ekf_frame_control_dev; csrc/ekf_control.hip) against the CPU oracle (oracle/ekf_oracle.c:457-523), an
extended-precision truth (tests/ekf_truth.py) and the decision rules of tests/ekf_control_restatement.py.

Shapes: batch 3; trail lengths 20, 5 and 1 (n = 160, 55, 27: even, odd -- every other filter then starts on an odd double, so the
streaming pass has a scalar element in front or behind and pairs that straddle two columns -- and fewer columns than the
workgroup has threads) and trail 20 with two map points (n = 166). Bars: ||dm|| / ||m||, ||dP||_F / ||P||_F <= 1e-5 against the
oracle (test_gpu_ekf.py's), and the scale-aware bar of test_gpu_ekf_accuracy.py against the truth."""
import math

import numpy as np
import pytest

import ekf_control_restatement as R
import ekf_truth as tr
from hybvio_amd import capi

pytestmark = pytest.mark.gpu
TOL = 1e-5
FACTOR, FLOOR = 8.0, 64 * tr.EPS64
POS, VEL, ORI, BGA, BAT, CAM = 0, 3, 6, 10, 16, 20
SHAPES = [(20, 0), (5, 0), (1, 0), (20, 2)]                  # (cameraTrailLength, hybridMapSize)
KINDS = ("zupt", "zrupt", "position", "zero_height", "orientation", "pseudo_velocity")
PARAM_KEYS = [k for k, _ in capi.EkfParams._fields_]


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def same_params(oracle, **over):
    po, pg = oracle.ekf_default_params(**over), capi.ekf_default_params(**over)
    for k in PARAM_KEYS:
        assert getattr(po, k) == getattr(pg, k), k
    return po, pg


def random_state(rng, n, trail, scale=1e2):
    """The recipe of tests/test_gpu_ekf.py:33-40."""
    m = rng.normal(size=n)
    m[ORI:ORI + 4] /= np.linalg.norm(m[ORI:ORI + 4])
    m[BAT:BAT + 3] = 1 + 0.01 * rng.normal(size=3)
    for c in range(trail):
        m[CAM + 7 * c + 3: CAM + 7 * c + 7] /= np.linalg.norm(m[CAM + 7 * c + 3: CAM + 7 * c + 7])
    A = rng.normal(size=(n, n))
    return m, scale * (A @ A.T / n + 0.1 * np.eye(n))


@pytest.fixture()
def ctx():
    import torch
    c = capi.Context(width=64, height=64, levels=1, pool_size=1)
    c.set_stream(torch.cuda.current_stream().cuda_stream)     # the tests' torch tensors and the library share one stream
    yield c
    torch.cuda.synchronize()
    c.close()


def make_pair(oracle, ctx, rng, trail, hyb=0, batch=3):
    po, pg = same_params(oracle, cameraTrailLength=trail, hybridMapSize=hyb)
    g = capi.EkfBatch(ctx, pg, batch)
    assert g.n == 20 + 7 * trail + 3 * hyb
    os_ = []
    for b in range(batch):
        o = oracle.Ekf(po)
        m, P = random_state(rng, o.n, trail)
        o.set_state(m); o.set_cov(P)
        g.set_state(b, m, P)
        os_.append(o)
    return po, os_, g


def dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def run_kind(kind, g, os_, ns, rng, active=None, applied=None):
    """One update kind on the device batch and on the oracle filters where `active` (None: all) is set. ns = noiseScale^2."""
    B = g.batch
    on = [True] * B if active is None else [bool(x) for x in active]
    act = dev(active, np.uint8) if active is not None else None
    kw = dict(active_dev=act.data_ptr() if act is not None else 0, applied_dev=applied.data_ptr() if applied is not None else 0)
    keep = [act]
    if kind == "zupt":                                       # per-filter R through r_dev
        r = 1e-7 * (1 + np.arange(B))
        rd = dev(r * ns); keep.append(rd)
        g.block_update_dev(VEL, 3, r_dev=rd.data_ptr(), **kw)
        for b, o in enumerate(os_):
            if on[b]:
                o.update_zupt(float(r[b]))
    elif kind == "zrupt":
        xg = rng.normal(0, 0.1, (B, 3))
        y = dev(xg); keep.append(y)
        g.block_update_dev(BGA, 3, y_dev=y.data_ptr(), r0=g.params.rotationZuptR * ns, **kw)
        for b, o in enumerate(os_):
            if on[b]:
                o.update_zrupt(xg[b])
    elif kind == "position":
        pos = rng.normal(size=(B, 3))
        y = dev(pos); keep.append(y)
        g.block_update_dev(POS, 3, y_dev=y.data_ptr(), r0=1e-3 * ns, **kw)
        g.symmetrize()
        for b, o in enumerate(os_):
            if on[b]:
                o.update_position(pos[b], 1e-3)
    elif kind == "zero_height":
        g.block_update_dev(POS + 2, 1, r0=1e-2 * ns, **kw)
        g.symmetrize()
        for b, o in enumerate(os_):
            if on[b]:
                o.update_zero_height(1e-2)
    elif kind == "orientation":
        q = rng.normal(size=(B, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
        y = dev(q); keep.append(y)
        g.block_update_dev(ORI, 4, y_dev=y.data_ptr(), r0=1e-2 * ns, normalize_all=True, **kw)
        g.symmetrize()
        for b, o in enumerate(os_):
            if on[b]:
                o.update_orientation(q[b], 1e-2)
    else:
        g.pseudo_velocity_dev(-1.0, 0.5, 1e-4, **kw)
        for b, o in enumerate(os_):
            if on[b]:
                o.update_pseudo_velocity(0.5, 1e-4)
    g.ctx.synchronize()
    return keep


@pytest.mark.parametrize("trail,hyb", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_update_parity_with_one_filter_masked_out(oracle, ctx, kind, trail, hyb):
    import torch
    rng = np.random.default_rng([KINDS.index(kind), trail, hyb])
    po, os_, g = make_pair(oracle, ctx, rng, trail, hyb)
    ns = po.noiseScale ** 2
    before = [g.get_state(b) for b in range(3)]
    applied = torch.full((3,), 7, dtype=torch.uint8, device="cuda")
    run_kind(kind, g, os_, ns, rng, active=[1, 0, 1], applied=applied)
    assert applied.cpu().tolist() == [1, 0, 1]
    for b, o in enumerate(os_):
        m, P = g.get_state(b)
        if b == 1:
            if kind in ("position", "zero_height", "orientation"):      # (hv_ekf_symmetrize has no mask)
                assert np.array_equal(m, before[b][0]) and np.array_equal(P, 0.5 * (before[b][1] + before[b][1].T))
            else:
                assert np.array_equal(m, before[b][0]) and np.array_equal(P, before[b][1])
            continue
        print(f"PARITY {kind} trail={trail} hyb={hyb} filter {b}: rel(m) {rel(m, o.m):.2e} rel(P) {rel(P, o.P):.2e}")
        assert rel(m, o.m) <= TOL and rel(P, o.P) <= TOL, (b, rel(m, o.m), rel(P, o.P))
        assert not np.array_equal(P, before[b][1])
    g.close()


def test_masked_filter_is_untouched_without_the_symmetrisation(oracle, ctx):
    """The block update itself leaves a masked-out filter bit-identical, also for the kinds the parity test follows with
    hv_ekf_symmetrize; all filters active and no flags is the NULL form of both arrays."""
    rng = np.random.default_rng(5)
    po, os_, g = make_pair(oracle, ctx, rng, 5)
    before = [g.get_state(b) for b in range(3)]
    act = dev([0, 1, 0], np.uint8)
    g.block_update_dev(ORI, 4, r0=1e-2, active_dev=act.data_ptr(), normalize_all=True)
    g.block_update_dev(POS + 2, 1, r0=1e-2, active_dev=act.data_ptr())
    ctx.synchronize()
    for b in (0, 2):
        m, P = g.get_state(b)
        assert np.array_equal(m, before[b][0]) and np.array_equal(P, before[b][1])
    assert not np.array_equal(g.get_state(1)[1], before[1][1])
    g.block_update_dev(VEL, 3, r0=1e-7)
    ctx.synchronize()
    for b in range(3):
        assert not np.array_equal(g.get_state(b)[1], before[b][1])
    g.close()


# ---- accuracy on the scale-aware bar ----

def truth_update(m, P, col0, kc, y, r, trail, W=None, v=None, normalize_all=False, symmetrize=False):
    """update() + updateCommon() (ekf.cpp:25-32, 57-82) for H = W E in extended precision, the reference's operands: HP from the
    rows of P, S from HP's columns, K' = S^-1 HP, P -= K HP; ORI normalised, the trail only for updateOrientation."""
    LD = tr.LD
    m, P = np.array(m, LD), np.array(P, LD)
    rows = P[col0:col0 + kc, :]
    if W is None:
        HP, S = rows.copy(), rows[:, col0:col0 + kc].copy()
        v = np.asarray(y, LD) - m[col0:col0 + kc]
    else:
        W = np.asarray(W, LD).reshape(1, kc)
        HP = W @ rows
        S = HP[:, col0:col0 + kc] @ W.T
        v = np.asarray([v], LD)
    S[np.diag_indices(S.shape[0])] += LD(r)
    X = tr.spd_solve(tr.chol(S), HP)
    m = m + X.T @ v
    P = P - X.T @ HP
    for o in [ORI] + ([CAM + 7 * c + 3 for c in range(trail)] if normalize_all else []):
        nn = np.sqrt(m[o:o + 4] @ m[o:o + 4])
        if nn > 0:
            m[o:o + 4] /= nn
    if symmetrize:
        P = (P + P.T) / 2
    return m, P


@pytest.fixture(scope="module")
def filters(oracle):
    """The oracle's closed loops, run once and left unchanged: {trail: (params, [(frame, m, P)])}, every regime's snapshots."""
    out = {}
    for trail in (20, 5):
        params, snaps = tr.realistic_filters(oracle, np.random.default_rng(77 + trail), trail=trail)
        out[trail] = (params, [s for r in tr.REGIMES for s in snaps[r]])
    return out


@pytest.mark.parametrize("trail", (20, 5))
@pytest.mark.parametrize("kind", KINDS)
def test_update_accuracy_on_running_covariances(oracle, ctx, filters, kind, trail):
    """Every update kind on covariances as a running filter holds them (diagonal from 1e-8 to 1e8): scaled_err and scaled_err_m
    of the device <= max(8 x the oracle's, 64 eps) against the extended-precision truth."""
    params, snaps = filters[trail]
    B = len(snaps)
    ns = params.noiseScale ** 2
    rng = np.random.default_rng([KINDS.index(kind), trail, 9])
    po, pg = same_params(oracle, cameraTrailLength=trail)
    g = capi.EkfBatch(ctx, pg, B)
    os_ = []
    for b, (_, m, P) in enumerate(snaps):
        g.set_state(b, m, P)
        os_.append(tr.oracle_filter(oracle, params, m, P))
    truths = []
    keep = None
    if kind == "zupt":
        g.block_update_dev(VEL, 3, r0=1e-7 * ns)
        for (_, m, P), o in zip(snaps, os_):
            o.update_zupt(1e-7)
            truths.append(truth_update(m, P, VEL, 3, np.zeros(3), 1e-7 * ns, trail))
    elif kind == "zrupt":
        xg = rng.normal(0, 0.01, (B, 3)); keep = dev(xg)
        g.block_update_dev(BGA, 3, y_dev=keep.data_ptr(), r0=params.rotationZuptR * ns)
        for b, ((_, m, P), o) in enumerate(zip(snaps, os_)):
            o.update_zrupt(xg[b])
            truths.append(truth_update(m, P, BGA, 3, xg[b], params.rotationZuptR * ns, trail))
    elif kind == "position":
        pos = np.stack([m[POS:POS + 3] for _, m, _ in snaps]) + rng.normal(0, 0.01, (B, 3)); keep = dev(pos)
        g.block_update_dev(POS, 3, y_dev=keep.data_ptr(), r0=1e-3 * ns); g.symmetrize()
        for b, ((_, m, P), o) in enumerate(zip(snaps, os_)):
            o.update_position(pos[b], 1e-3)
            truths.append(truth_update(m, P, POS, 3, pos[b], 1e-3 * ns, trail, symmetrize=True))
    elif kind == "zero_height":
        g.block_update_dev(POS + 2, 1, r0=1e-2 * ns); g.symmetrize()
        for (_, m, P), o in zip(snaps, os_):
            o.update_zero_height(1e-2)
            truths.append(truth_update(m, P, POS + 2, 1, np.zeros(1), 1e-2 * ns, trail, symmetrize=True))
    elif kind == "orientation":
        q = np.stack([m[ORI:ORI + 4] for _, m, _ in snaps]) + rng.normal(0, 0.01, (B, 4))
        q /= np.linalg.norm(q, axis=1, keepdims=True); keep = dev(q)
        g.block_update_dev(ORI, 4, y_dev=keep.data_ptr(), r0=1e-2 * ns, normalize_all=True); g.symmetrize()
        for b, ((_, m, P), o) in enumerate(zip(snaps, os_)):
            o.update_orientation(q[b], 1e-2)
            truths.append(truth_update(m, P, ORI, 4, q[b], 1e-2 * ns, trail, normalize_all=True, symmetrize=True))
    else:
        applied = dev(np.full(B, 7), np.uint8)
        g.pseudo_velocity_dev(-1.0, 0.0, 1e-4, applied_dev=applied.data_ptr())
        ctx.synchronize()
        assert applied.cpu().tolist() == [1] * B
        for (_, m, P), o in zip(snaps, os_):
            o.update_pseudo_velocity(0.0, 1e-4)
            h = math.sqrt(m[VEL] * m[VEL] + m[VEL + 1] * m[VEL + 1])        # binary64, as both implementations form it
            truths.append(truth_update(m, P, VEL, 2, None, 1e-4 * ns, trail, W=[m[VEL] / h, m[VEL + 1] / h], v=0.0 - h))
    ctx.synchronize()
    failures = []
    for b, ((frame, _, _), o, (mT, T)) in enumerate(zip(snaps, os_, truths)):
        mg, Pg = g.get_state(b)
        eg, eo = tr.scaled_err(Pg, T), tr.scaled_err(o.P, T)
        gm, om = tr.scaled_err_m(mg, mT, T), tr.scaled_err_m(o.m, mT, T)
        print(f"ACC {kind} trail={trail} frame={frame}: P scaled error device {eg:.2e} oracle {eo:.2e}; m device {gm:.2e} oracle {om:.2e}")
        if not eg <= max(FACTOR * eo, FLOOR):
            failures.append(f"frame {frame}: P {eg:.2e} > max(8 x {eo:.2e}, 64 eps)")
        if not gm <= max(FACTOR * om, FLOOR):
            failures.append(f"frame {frame}: m {gm:.2e} > max(8 x {om:.2e}, 64 eps)")
    g.close()
    assert not failures, f"{kind} trail={trail}: " + " | ".join(failures)


# ---- gates, refusals, arguments ----

def test_pseudo_velocity_gates(oracle, ctx):
    """h <= 1e-7, h <= limit, h > limit: the applied flags exactly, the skipped filters bit-identical; limit < 0: no limit test."""
    rng = np.random.default_rng(11)
    for limit, speeds, want in ((1.4, [(0.0, 0.0), (0.3, 0.4), (3.0, 4.0)], [0, 0, 1]),
                                (-1.0, [(1e-7, 0.0), (0.3, 0.4), (0.0, 1.0000001e-7)], [0, 1, 1]),
                                (5.0, [(3.0, 4.0), (3.0, 4.000001), (0.0, 0.0)], [0, 1, 0])):      # (9 + 16 = 25: h is 5 exactly)
        hs = [math.sqrt(vx * vx + vy * vy) for vx, vy in speeds]
        assert want == [int(R.pseudo_velocity_due(h) and not (limit >= 0 and h <= limit)) for h in hs]
        po, os_, g = make_pair(oracle, ctx, rng, 5)
        before = []
        for b, (vx, vy) in enumerate(speeds):
            m, P = g.get_state(b)
            m[VEL], m[VEL + 1] = vx, vy
            g.set_state(b, m, P); os_[b].set_state(m)
            before.append((m, P))
        applied = dev(np.full(3, 7), np.uint8)
        g.pseudo_velocity_dev(limit, 0.25, 1e-4, applied_dev=applied.data_ptr())
        ctx.synchronize()
        assert applied.cpu().tolist() == want, (limit, applied.cpu().tolist())
        for b, o in enumerate(os_):
            m, P = g.get_state(b)
            if want[b]:
                o.update_pseudo_velocity(0.25, 1e-4)
                assert rel(m, o.m) <= TOL and rel(P, o.P) <= TOL
            else:
                assert np.array_equal(m, before[b][0]) and np.array_equal(P, before[b][1])
        g.close()


def test_non_positive_pivot_leaves_the_filter_untouched(oracle, ctx):
    """A covariance whose VEL block is negative: S = P[VEL, VEL] + r I has no positive pivot. The filter is untouched and
    applied = 0; its neighbours are updated. A second case fails at the LAST pivot only."""
    rng = np.random.default_rng(13)
    po, os_, g = make_pair(oracle, ctx, rng, 5)
    states = [g.get_state(b) for b in range(3)]
    states[0][1][VEL:VEL + 3, VEL:VEL + 3] = -np.eye(3)
    states[2][1][VEL + 2, VEL + 2] = -50.0
    for b in (0, 2):
        g.set_state(b, *states[b])
    applied = dev(np.full(3, 7), np.uint8)
    g.block_update_dev(VEL, 3, r0=1e-7, applied_dev=applied.data_ptr())
    ctx.synchronize()
    assert applied.cpu().tolist() == [0, 1, 0]
    for b in (0, 2):
        m, P = g.get_state(b)
        assert np.array_equal(m, states[b][0]) and np.array_equal(P, states[b][1])
    assert not np.array_equal(g.get_state(1)[1], states[1][1])
    g.close()


def test_argument_checks_with_a_live_filter(oracle, ctx):
    import ctypes as C
    L = capi.lib()
    g = capi.EkfBatch(ctx, capi.ekf_default_params(cameraTrailLength=1), 2)
    for col0, rows in ((VEL, 0), (VEL, 5), (-1, 3), (g.n - 2, 3), (g.n, 1)):
        assert L.hv_ekf_block_update_dev(g._h, col0, rows, None, None, 1e-7, None, 0, None) == -1, (col0, rows)
    ctl = capi.EkfControl(2)
    p = capi.ekf_control_default_params()
    t = dev(np.zeros(2)); kf = dev(np.zeros(2), np.int32)
    for k, _ in capi.EkfControlTable._fields_:
        bad = capi.EkfControlTable(*(None if k2 == k else getattr(ctl.table, k2) for k2, _ in capi.EkfControlTable._fields_))
        assert L.hv_ekf_control_init_dev(g._h, C.byref(bad)) == -1
        assert L.hv_ekf_imu_control_dev(g._h, C.byref(p), C.byref(bad), C.c_void_p(t.data_ptr()), None) == -1
        assert L.hv_ekf_frame_control_dev(g._h, C.byref(p), C.byref(bad), C.c_void_p(t.data_ptr()), C.c_void_p(kf.data_ptr()),
                                          None, None, None, None, None) == -1
    assert L.hv_ekf_frame_control_dev(g._h, C.byref(p), C.byref(ctl.table), None, C.c_void_p(kf.data_ptr()), None, None, None, None, None) == -1
    assert L.hv_ekf_frame_control_dev(g._h, C.byref(p), C.byref(ctl.table), C.c_void_p(t.data_ptr()), None, None, None, None, None, None) == -1
    g.control_init_dev(ctl)
    ctx.synchronize()
    assert ctl.zupt_time.cpu().tolist() == [-1.0, -1.0] and ctl.init_zupt_time.cpu().tolist() == [-1.0, -1.0]
    assert ctl.was_stationary.cpu().tolist() == [0, 0] and ctl.frames_since_keyframe.cpu().tolist() == [0, 0]
    g.close()


def test_undo_augment_dev_equals_undo_augment(oracle, ctx):
    """The same mask from the device and from the host: bit for bit, masked-out filters carried over."""
    rng = np.random.default_rng(17)
    for trail, hyb in ((5, 0), (20, 2)):
        _, _, g1 = make_pair(oracle, ctx, rng, trail, hyb)
        g2 = capi.EkfBatch(ctx, g1.params, 3)
        for b in range(3):
            g2.set_state(b, *g1.get_state(b))
        mask = np.array([1, 0, 1], np.uint8)
        d = dev(mask)
        g1.undo_augment_dev(d.data_ptr())
        g2.undo_augment(mask)
        ctx.synchronize()
        for b in range(3):
            (m1, P1), (m2, P2) = g1.get_state(b), g2.get_state(b)
            assert np.array_equal(m1, m2) and np.array_equal(P1, P2)
        g1.undo_augment_dev(0); g2.undo_augment(None)
        ctx.synchronize()
        for b in range(3):
            (m1, P1), (m2, P2) = g1.get_state(b), g2.get_state(b)
            assert np.array_equal(m1, m2) and np.array_equal(P1, P2)
        g1.close(); g2.close()


# ---- closed loop ----

def keyframe_schedule(frame):
    """Filter 0: always a keyframe. Filter 1: no keyframe on frames 4-16 -- at a 0.06 s period it sees not yet stationary, the
    ZUPT applied, rate-limited, applied again. Filter 2 alternates, starting with a keyframe: the reference never undoes an
    augmentation it has not made (the oracle's augmentCount would go negative)."""
    return [1, 0 if 4 <= frame <= 16 else 1, 1 - frame % 2]


@pytest.mark.parametrize("controls", (False, True))
def test_closed_loop_20_frames(oracle, ctx, controls):
    """Per frame on the device: predict_n_dev of three samples, normalize_quaternions(only_current), imu_control_dev,
    frame_control_dev, undo_augment_dev(undo_active), augment_dev; on the oracle the same through the restatement's decisions
    and the oracle's own rate limiters. Every integer and flag array equals the restatement at every frame, the state agrees
    to 1e-5 at the end. controls: useDecayingZeroVelocityUpdate and usePseudoVelocity on (the limit lowered to 0.05 m/s and a
    horizontal acceleration, so that the pseudo-velocity update is reached between two init-ZUPTs)."""
    import torch
    B, trail, frames, dt = 3, 5, 20, 0.02
    rng = np.random.default_rng(20 + controls)
    po, pg = same_params(oracle, cameraTrailLength=trail)
    rp = R.Params(useDecayingZeroVelocityUpdate=controls, usePseudoVelocity=controls, pseudoVelocityLimit=0.05 if controls else 1.4)
    cp = capi.ekf_control_default_params(useDecayingZeroVelocityUpdate=int(controls), usePseudoVelocity=int(controls),
                                         pseudoVelocityLimit=rp.pseudoVelocityLimit)
    g = capi.EkfBatch(ctx, pg, B)
    acc0 = np.array([0.0, 0.0, 9.81])
    os_, st = [], [R.State() for _ in range(B)]
    for b in range(B):
        o = oracle.Ekf(po)
        o.initialize_orientation(acc0)
        o.set_first_sample_time(0.0)
        g.set_state(b, o.m.copy(), o.P.copy())
        os_.append(o)
    ctl = capi.EkfControl(B)
    g.control_init_dev(ctl)
    kf_out = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    undo, stat, appl = (torch.full((B,), 7, dtype=torch.uint8, device="cuda") for _ in range(3))
    d_dt = dev(np.full((3, B), dt))
    seen = {}
    step = 0
    for frame in range(frames):
        gy = rng.normal(0, 0.02, (3, B, 3))
        ac = acc0 + rng.normal(0, 0.05, (3, B, 3)) + ([2.0, 0.0, 0.0] if controls else [0.0, 0.0, 0.0])
        d_gy, d_ac = dev(gy), dev(ac)
        g.predict_n_dev(3, d_dt.data_ptr(), d_gy.data_ptr(), d_ac.data_ptr())
        g.normalize_quaternions(True)
        for s in range(3):
            step += 1
            for b, o in enumerate(os_):
                o.predict(step * dt, gy[s, b], ac[s, b])
        time = step * dt
        kf = keyframe_schedule(frame)
        d_time, d_kf = dev(np.full(B, time)), dev(kf, np.int32)
        g.imu_control_dev(cp, ctl, d_time.data_ptr())
        g.frame_control_dev(cp, ctl, d_time.data_ptr(), d_kf.data_ptr(), keyframe_out_dev=kf_out.data_ptr(),
                            undo_active_dev=undo.data_ptr(), stationary_dev=stat.data_ptr(), applied_dev=appl.data_ptr())
        g.undo_augment_dev(undo.data_ptr())
        g.augment_dev()
        want = {"keyframe_out": [], "undo": [], "stationary": [], "zupt": []}
        for b, o in enumerate(os_):
            o.normalize_quaternions(1)
            expired = controls and st[b].was_stationary
            if R.imu_init_zupt(rp, st[b], time):
                o.update_zupt_initialization()
                seen["init-ZUPT applied"] = True
            elif expired:
                seen["init-ZUPT expired"] = True
            h = math.sqrt(o.m[VEL] * o.m[VEL] + o.m[VEL + 1] * o.m[VEL + 1])
            if R.imu_pseudo_velocity(rp, h):
                o.update_pseudo_velocity(rp.pseudoVelocityTarget, rp.pseudoVelocityR)
                seen["pseudo-velocity applied"] = True
            d = R.frame_control(rp, st[b], time, bool(kf[b]))
            if d["zupt"]:
                o.update_zupt(rp.visualZuptR)
            seen["applied" if d["zupt"] else ("rate-limited" if d["stationary"] else "not stationary")] = True
            if d["undo"]:
                o.update_undo_augmentation()
            seen["undo" if d["undo"] else "no undo"] = True
            o.update_visual_pose_augmentation(-1)
            for k in want:
                want[k].append(int(d[k]))
        ctx.synchronize()
        got = {"keyframe_out": kf_out, "undo": undo, "stationary": stat, "zupt": appl}
        for k in want:
            assert got[k].cpu().tolist() == want[k], (frame, k, got[k].cpu().tolist(), want[k])
        for k in ("zupt_time", "init_zupt_time", "was_stationary", "frames_since_keyframe"):
            assert getattr(ctl, k).cpu().tolist() == [getattr(s, k) for s in st], (frame, k)
    need = {"applied", "rate-limited", "not stationary", "undo", "no undo"}
    if controls:
        need |= {"init-ZUPT applied", "init-ZUPT expired", "pseudo-velocity applied"}
    assert need <= set(seen), sorted(seen)
    for b, o in enumerate(os_):
        m, P = g.get_state(b)
        print(f"LOOP controls={controls} filter {b}: rel(m) {rel(m, o.m):.2e} rel(P) {rel(P, o.P):.2e}")
        assert rel(m, o.m) <= TOL and rel(P, o.P) <= TOL, (b, rel(m, o.m), rel(P, o.P))
    g.close()
