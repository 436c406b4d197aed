"""GPU tests of the session lifecycle entries (hv_session_init_dev, hv_session_imu_dev, hv_session_status_dev, hv_session_reset_dev;
csrc/session.hip) against the literal restatement tests/session_restatement.py and the CPU oracle (oracle/ekf_oracle.c).

Shapes: batch 5, of which the sets 0, 2 and 4 reset and 1 and 3 do not; cameraTrailLength 3 (n = 41, odd: every other filter's
covariance starts on an odd double) and 20 (n = 160); maxTracks 8; a ring of W = 4 flags (targetFps 2), which wraps within ten
frames, and W = 60 (the defaults) once.
Bars: clocks, flags, rings and every table slice are bit-equal. initializeOrientation: q within 1e-15 absolute of the oracle (a few
rounded operations on components of at most 1; the kernels may contract), its P block within 1e-15 relative. Keep-pose reset: every
diagonal block of P within 32 * 2^-53 of the block's largest magnitude (an entry is at most four products of three bounded factors,
summed), everything outside the blocks bit-equal; the chain agrees with the oracle at the project's EKF bar, 1e-5 relative."""
import ctypes as C

import numpy as np
import pytest

import session_restatement as R
from hybvio_amd import capi

pytestmark = pytest.mark.gpu
B, M = 5, 8
RESET_SETS, KEPT_SETS = (0, 2, 4), (1, 3)
POS, VEL, ORI, BAT, CAM = 0, 3, 6, 16, 20
U = 2.0 ** -53
TOL = 1e-5
PARAM_KEYS = [k for k, _ in capi.EkfParams._fields_]


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


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


def blocks(trail):
    return [(POS, 3), (VEL, 3), (ORI, 4)] + [(CAM + 7 * c + o, k) for c in range(trail) for o, k in ((0, 3), (3, 4))]


@pytest.fixture()
def ctx():
    import torch
    c = capi.Context(width=64, height=64, levels=1, pool_size=1)
    c.set_stream(torch.cuda.current_stream().cuda_stream)     # the tests' torch tensors and the library share one stream
    yield c
    torch.cuda.synchronize()
    c.close()


def trail_params(trail):
    return capi.trail_index_default_params(cameraTrailLength=trail, cameraTrailHanoiLength=min(3, trail - 2), maxTracks=M)


class World:
    """Everything a reset touches besides the filter, for B sets: session, control block, track table, trail index."""

    def __init__(self, trail, W):
        import torch
        self.torch = torch
        self.tp = capi.track_table_default_params(maxTracks=M)
        self.ip = trail_params(trail)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        self.tm = dict(n_tracks=z(B, torch.int32), ids=z((B, M), torch.int32), xy=z((B, M, 2), torch.float32),
                       second_xy=z((B, M, 2), torch.float32), status=z((B, M), torch.int32), blacklist=z((B, M), torch.uint8),
                       kf_xy=z((B, M, 2), torch.float32), kf_valid=z((B, M), torch.uint8), frame_num=z(B, torch.int32),
                       mask_steps=z(B, torch.int32), mask_radius=z(B, torch.int32), frame_flags=z(B, torch.uint8))
        self.table = capi.track_table(**{k: v.data_ptr() for k, v in self.tm.items()})
        self.trail = capi.TrailIndex(B, self.ip)
        self.ctl = capi.EkfControl(B)
        self.cm = {k: getattr(self.ctl, k) for k, _ in capi.EkfControlTable._fields_}
        self.ses = capi.session_state(B, W)
        assert isinstance(self.ses, capi.Session) and self.ses.m["good_ring"].shape == (B, W)

    def groups(self):
        return {"table": self.tm, "trail": self.trail.m, "ctl": self.cm, "session": self.ses.m}

    def fill_sentinels(self, seed):
        """A different, reproducible pattern in every array (flags included: a not-reset set must keep whatever it holds)."""
        torch = self.torch
        gen = torch.Generator(device="cpu").manual_seed(seed)
        for gname, group in self.groups().items():
            for k, t in group.items():
                if t.dtype in (torch.float32, torch.float64):
                    v = torch.rand(t.shape, generator=gen, dtype=torch.float64) * 100 + 1
                else:
                    v = torch.randint(1, 100, t.shape, generator=gen)
                t.copy_(v.to(t.dtype))

    def snapshot(self):
        self.torch.cuda.synchronize()
        return {g: {k: t.cpu().numpy().copy() for k, t in group.items()} for g, group in self.groups().items()}

    def init_all(self, ctx, g, sp):
        ctx.tracks_init_batch_dev(B, self.table, params=self.tp)
        ctx.trail_init_batch_dev(B, self.trail.table, params=self.ip)
        g.control_init_dev(self.ctl)
        g.session_init_dev(sp, self.ses)

    def reset(self, g, sp, kind_dev):
        g.session_reset_dev(sp, self.ses, self.ctl, self.tp, self.table, self.ip, self.trail.table, kind_dev.data_ptr())


def session_arrays(ctls, W):
    """The hv_session arrays the restatement's Control objects stand for."""
    out = {k: [] for k, _ in capi.SessionState._fields_}
    for c in ctls:
        s = c.session
        out["good_ring"].append(s.counter.buffer.copy())
        out["ring_head"].append(s.counter.head); out["ring_entries"].append(s.counter.entries)
        out["tracking_status"].append(s.tracking_status); out["control_status"].append(c.control_status)
        out["last_reset_time"].append(c.last_reset_time)
        out["first_sample"].append(int(s.clock.first_sample)); out["first_sample_t"].append(s.clock.first_sample_t)
        out["prev_sample_t"].append(s.clock.prev_sample_t); out["time"].append(s.clock.time)
        out["initialized_orientation"].append(int(s.initialized_orientation))
    return out


def assert_session_equal(ses, ctls, what):
    import torch
    torch.cuda.synchronize()
    want = session_arrays(ctls, ses.W)
    for k, t in ses.m.items():
        got = t.cpu().numpy()
        assert np.array_equal(got, np.asarray(want[k], got.dtype)), (what, k, got.tolist(), want[k])


def get_filter(g, b):
    """m, P, Q, dydx of filter b."""
    m, P = g.get_state(b)
    Q = np.zeros(144)
    assert capi.lib().hv_ekf_get_process_noise(g._h, b, Q.ctypes.data_as(capi.f64p)) == 0
    return m, P, Q, g.get_dydx(b)


# ---- imu ---------------------------------------------------------------------------------------------------------------------

ACC = {0: (0.3, -0.2, 9.7), 1: (0.0, 0.0, -5.0), 2: (0.0, 0.0, 0.0), 3: (1.0, 2.0, 3.0), 4: (0.4, 0.1, 9.9)}      # ordinary, antiparallel, zero


@pytest.mark.parametrize("trail", [3, 20])
@pytest.mark.parametrize("n_samples", [1, 3, 32])
def test_imu_clock_and_orientation(oracle, ctx, trail, n_samples):
    """Set 0: a first sample, ordinary acceleration (and, from three samples on, a repeated timestamp); 1: antiparallel; 2: zero
    acceleration; 3: masked out, with a stored clock; 4: a session that is past its first sample and has its orientation, whose first
    timestamp repeats the previous one."""
    import torch
    rng = np.random.default_rng([trail, n_samples])
    po, pg = same_params(oracle, cameraTrailLength=trail)
    g = capi.EkfBatch(ctx, pg, B)
    sp = capi.session_default_params(targetFps=2.0)
    rp = R.Params(targetFps=2.0)
    w = World(trail, 4)
    g.session_init_dev(sp, w.ses)
    states = [random_state(rng, g.n, trail) for _ in range(B)]
    for b, (m, P) in enumerate(states):
        g.set_state(b, m, P)
    ctls = [R.Control(rp) for _ in range(B)]
    # sets 3 and 4 carry a clock already
    for b, (first_t, prev_t) in ((3, (1.5, 4.75)), (4, (2.0, 7.25))):
        c = ctls[b].session.clock
        c.first_sample, c.first_sample_t, c.prev_sample_t, c.time = False, np.float64(first_t), np.float64(prev_t), np.float64(prev_t) - np.float64(first_t)
        ctls[b].session.initialized_orientation = b == 4
        for k, v in (("first_sample", 0), ("first_sample_t", first_t), ("prev_sample_t", prev_t), ("time", prev_t - first_t),
                     ("initialized_orientation", int(b == 4))):
            w.ses.m[k][b] = v
    t = np.zeros((n_samples, B))
    for b, base in enumerate((100.0, 0.1, 33.3, 5.0, 7.25)):
        t[:, b] = base + 0.005 * np.arange(n_samples) * (1 + 0.1 * b)
    if n_samples >= 3:
        t[2, 0] = t[1, 0]                                      # a repeated timestamp: dt = 0
    acc = np.zeros((n_samples, B, 3))
    for b in range(B):
        acc[:, b] = ACC[b]
    acc[1:] += rng.normal(0, 0.1, acc[1:].shape)               # only the first sample may set the orientation
    active = np.array([1, 1, 1, 0, 1], np.uint8)
    d_t, d_acc, d_act = dev(t), dev(acc), dev(active)
    dt_out = torch.full((n_samples, B), -7.0, dtype=torch.float64, device="cuda")
    time_out = torch.full((n_samples, B), -7.0, dtype=torch.float64, device="cuda")
    g.session_imu_dev(w.ses, n_samples, d_t.data_ptr(), d_acc.data_ptr(), dt_out.data_ptr(), time_out.data_ptr(), active_dev=d_act.data_ptr())
    ctx.synchronize()

    want_dt, want_time, want_q = np.zeros((n_samples, B)), np.zeros((n_samples, B)), {}
    for b in range(B):
        for s in range(n_samples):
            if not active[b]:
                want_dt[s, b], want_time[s, b] = 0.0, ctls[b].session.clock.time
                continue
            q, dt = ctls[b].session.imu(t[s, b], acc[s, b], po.gravity)
            if q is not None:
                assert s == 0
                want_q[b] = q
            want_dt[s, b], want_time[s, b] = dt, ctls[b].session.clock.time
    assert sorted(want_q) == [0, 1, 2]
    assert np.array_equal(dt_out.cpu().numpy(), want_dt) and np.array_equal(time_out.cpu().numpy(), want_time)
    if n_samples >= 3:
        assert want_dt[2, 0] == 0.0 and want_dt[0, 0] == 0.0 and want_dt[1, 0] > 0.0
    assert want_dt[0, 4] == 0.0                                # the repeat of the stored timestamp
    assert_session_equal(w.ses, ctls, "imu")

    for b, (m0, P0) in enumerate(states):
        m, P = g.get_state(b)
        if b not in want_q:
            assert np.array_equal(m, m0) and np.array_equal(P, P0), b      # masked out / already initialised: untouched
            continue
        if b == 2:                                             # the oracle divides by zero here: the zero-vector rule
            q_o, blk_o = np.array([np.sqrt(2.0) / 2, 0.0, 0.0, 0.0]), R.orientation_block(po)
        else:
            o = oracle.Ekf(po)
            o.initialize_orientation(acc[0, b])
            q_o, blk_o = np.array(o.m[ORI:ORI + 4]), np.array(o.P[ORI:ORI + 4, ORI:ORI + 4])
        assert np.abs(m[ORI:ORI + 4] - q_o).max() <= 1e-15, (b, m[ORI:ORI + 4], q_o)
        assert np.abs(want_q[b] - q_o).max() <= 1e-15
        assert np.abs(P[ORI:ORI + 4, ORI:ORI + 4] - blk_o).max() <= 1e-15 * np.abs(blk_o).max()
        m_rest, P_rest = m.copy(), P.copy()
        m_rest[ORI:ORI + 4] = m0[ORI:ORI + 4]
        P_rest[ORI:ORI + 4, ORI:ORI + 4] = P0[ORI:ORI + 4, ORI:ORI + 4]
        assert np.array_equal(m_rest, m0) and np.array_equal(P_rest, P0), b    # every other entry bit-unchanged
    g.close()


# ---- status ------------------------------------------------------------------------------------------------------------------

def scripted_flags(frames, seed):
    """good[f][b], full[f][b]: a different script in every set."""
    rng = np.random.default_rng(seed)
    good, full = np.zeros((frames, B), np.uint8), np.ones((frames, B), np.uint8)
    good[:, 0] = 1                                             # always good: TRACKING at the first consulted mean
    good[:, 1] = 0                                             # never good: stays INIT
    good[:4, 2] = 1                                            # good, then bad: TRACKING, then LOST
    good[:, 3] = np.arange(frames) % 2
    full[:, 3] = (np.arange(frames) % 3 != 1)                  # a frame in three is not a full update: no put
    good[:, 4] = rng.integers(0, 2, frames)
    return good, full


SCENARIOS = {
    # name: (session parameters, frames, frame spacing, parameters switched after a frame)
    "defaults_w4": (dict(targetFps=2.0), 12, 0.5, {}),
    "reset_until_init_succeeds": (dict(targetFps=2.0, resetUntilInitSucceeds=1), 16, 0.5, {}),
    "reset_on_failed_tracking": (dict(targetFps=2.0, resetOnFailedTracking=1), 16, 0.5, {}),
    "failed_to_initialize_after_reset": (dict(targetFps=2.0, resetOnFailedTracking=1), 18, 0.5, {8: dict(resetOnFailedTracking=0)}),
    "freeze": (dict(targetFps=2.0, freezeOnFailedTracking=1), 12, 0.5, {}),
    "defaults_w60": (dict(), 40, 0.1, {}),
}


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_status_sequences_equal_the_restatement(ctx, name):
    """Per frame: one IMU sample (the clock), the status entry, and -- where it decided a reset -- the reset entry; after every call
    all state arrays and the three outputs equal the restatement's."""
    import torch
    over, frames, spacing, switch = SCENARIOS[name]
    trail = 3
    g = capi.EkfBatch(ctx, capi.ekf_default_params(cameraTrailLength=trail), B)
    sp, rp = capi.session_default_params(**over), R.Params(**over)
    W = capi.session_window(sp)
    assert W == R.window(rp) == (60 if name == "defaults_w60" else 4)
    w = World(trail, W)
    w.fill_sentinels(3)
    w.init_all(ctx, g, sp)
    ctls = [R.Control(rp) for _ in range(B)]
    assert_session_equal(w.ses, ctls, "init")
    good, full = scripted_flags(frames, 11)
    status = torch.full((B,), -9, dtype=torch.int32, device="cuda")
    frozen = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
    kind = torch.full((B,), -9, dtype=torch.int32, device="cuda")
    dt_out, time_out = torch.zeros((1, B), dtype=torch.float64, device="cuda"), torch.zeros((1, B), dtype=torch.float64, device="cuda")
    seen = set()
    for f in range(frames):
        if f in switch:
            for k, v in switch[f].items():
                setattr(sp, k, v); setattr(rp, k, v)
        t = np.full((1, B), 10.0 + spacing * f) + 0.01 * np.arange(B)
        acc = np.tile(np.array([0.1, 0.2, 9.8]), (1, B, 1))
        d_t, d_acc, d_good, d_full = dev(t), dev(acc), dev(good[f]), dev(full[f])
        g.session_imu_dev(w.ses, 1, d_t.data_ptr(), d_acc.data_ptr(), dt_out.data_ptr(), time_out.data_ptr())
        g.session_status_dev(sp, w.ses, d_good.data_ptr(), kind.data_ptr(), full_update_dev=d_full.data_ptr(), status_dev=status.data_ptr(),
                             frozen_dev=frozen.data_ptr())
        want = []
        for b, c in enumerate(ctls):
            c.session.imu(t[0, b], acc[0, b], 9.819)
            want.append(c.frame(bool(good[f, b]), bool(full[f, b])))
        assert_session_equal(w.ses, ctls, (name, f))
        assert status.cpu().tolist() == [x[0] for x in want], (name, f)
        assert frozen.cpu().tolist() == [int(x[1]) for x in want], (name, f)
        assert kind.cpu().tolist() == [x[2] for x in want], (name, f)
        seen |= {("kind", x[2]) for x in want} | {("frozen", x[1]) for x in want} | {("tracking", c.session.tracking_status) for c in ctls}
        seen |= {("wrapped", W) for c in ctls if c.session.counter.entries == W and c.session.counter.head != 0}
        if name == "defaults_w4" and f == 1:
            assert ctls[0].session.counter.entries == W // 2 and ctls[0].session.tracking_status == R.INIT      # the boundary: not consulted
        if name == "defaults_w4" and f == 2:
            assert ctls[0].session.tracking_status == R.TRACKING
        if any(x[2] for x in want):
            w.reset(g, sp, kind)
            for c, x in zip(ctls, want):
                if x[2]:
                    c.reset(x[2] == R.RESET_KEEP_POSE)
            assert_session_equal(w.ses, ctls, (name, f, "reset"))
    if name == "defaults_w4":
        assert seen >= {("tracking", R.INIT), ("tracking", R.TRACKING), ("tracking", R.LOST_TRACKING), ("wrapped", 4)}
        assert ("kind", 1) not in seen and ("kind", 2) not in seen and ("frozen", True) not in seen
    if name == "reset_until_init_succeeds":
        assert ("kind", R.RESET_FRESH) in seen and ("kind", R.RESET_KEEP_POSE) not in seen
    if name in ("reset_on_failed_tracking", "failed_to_initialize_after_reset"):
        assert ("kind", R.RESET_KEEP_POSE) in seen and ("kind", R.RESET_FRESH) not in seen
    if name == "failed_to_initialize_after_reset":             # the third rule: Control past INIT, the new session INIT, timer expired
        assert any(c.control_status != R.INIT and c.session.tracking_status == R.INIT and c.last_reset_time > 14.0 for c in ctls)
    if name == "freeze":
        assert ("frozen", True) in seen and ("frozen", False) in seen
    if name == "defaults_w60":
        assert ("tracking", R.TRACKING) in seen and ctls[0].session.counter.entries == 40
    g.close()


def test_status_without_the_optional_arrays(ctx):
    """full_update_dev NULL: every frame is a full update; status_dev and frozen_dev NULL: not written."""
    import torch
    g = capi.EkfBatch(ctx, capi.ekf_default_params(cameraTrailLength=3), B)
    sp, rp = capi.session_default_params(targetFps=2.0), R.Params(targetFps=2.0)
    w = World(3, 4)
    g.session_init_dev(sp, w.ses)
    ctls = [R.Control(rp) for _ in range(B)]
    kind = torch.full((B,), -9, dtype=torch.int32, device="cuda")
    for f in range(5):
        d_good = dev(np.array([1, 0, 1, 1, 0], np.uint8))
        g.session_status_dev(sp, w.ses, d_good.data_ptr(), kind.data_ptr())
        for b, c in enumerate(ctls):
            c.frame(bool([1, 0, 1, 1, 0][b]))
        assert_session_equal(w.ses, ctls, f)
        assert kind.cpu().tolist() == [0] * B
    g.close()


# ---- reset -------------------------------------------------------------------------------------------------------------------

def prepared_reset(oracle, ctx, trail, kinds, augments=0, seed=0):
    """A batch with random filters and sentinel patterns in every array, `augments` pose augmentations applied, then ONE reset launch
    with `kinds`. Returns what the tests compare."""
    import torch
    rng = np.random.default_rng([trail, seed])
    po, pg = same_params(oracle, cameraTrailLength=trail)
    g = capi.EkfBatch(ctx, pg, B)
    sp = capi.session_default_params(targetFps=2.0)
    w, w2 = World(trail, 4), World(trail, 4)
    w.fill_sentinels(5); w2.fill_sentinels(5)
    w2.init_all(ctx, g, sp)                                   # the second set of arrays: what the init entries write
    for b in range(B):
        g.set_state(b, *random_state(rng, g.n, trail))
    for _ in range(augments):
        g.augment_dev()                                       # P and P1 change places
    ctx.synchronize()
    before = [get_filter(g, b) for b in range(B)]
    snap0 = w.snapshot()
    kind = dev(np.array(kinds, np.int32))
    w.reset(g, sp, kind)
    ctx.synchronize()
    return po, pg, g, w, w2, before, snap0


def check_everything_but_the_filter(w, w2, snap0, kinds):
    snap, snap_init = w.snapshot(), w2.snapshot()
    reset_sets = [b for b, k in enumerate(kinds) if k in (1, 2)]
    for gname in ("table", "trail", "ctl"):
        for k in snap[gname]:
            for b in range(B):
                want = snap_init[gname][k][b] if b in reset_sets else snap0[gname][k][b]
                assert np.array_equal(snap[gname][k][b], want), (gname, k, b)
    s, s0 = snap["session"], snap0["session"]
    for b in range(B):
        if b not in reset_sets:
            for k in s:
                assert np.array_equal(s[k][b], s0[k][b]), (k, b)
            continue
        assert not s["good_ring"][b].any() and s["ring_head"][b] == 0 and s["ring_entries"][b] == 0
        assert s["tracking_status"][b] == R.INIT and s["first_sample"][b] == 1
        assert s["first_sample_t"][b] == -1.0 and s["prev_sample_t"][b] == -1.0 and s["time"][b] == 0.0
        assert s["initialized_orientation"][b] == (1 if kinds[b] == 2 else 0)
        assert s["control_status"][b] == s0["control_status"][b]                       # Control's: kept
        assert s["last_reset_time"][b] == s0["first_sample_t"][b] + s0["time"][b]      # the old clock


@pytest.mark.parametrize("trail,augments", [(3, 0), (20, 0), (3, 1), (20, 3)])
def test_reset_fresh_is_a_new_filter_and_new_tables(oracle, ctx, trail, augments):
    """Kind 1 in the sets 0, 2, 4 (set 3 holds a value that is no reset kind): m, P, Q and dydx bit-equal to a filter of a freshly
    created hv_ekf -- also after an odd number of augmentations, when the current covariance is the other buffer of the
    ping-pong --, the table, trail and control slices bit-equal to what the three init entries write, everything else untouched."""
    kinds = [1, 0, 1, 3, 1]
    po, pg, g, w, w2, before, snap0 = prepared_reset(oracle, ctx, trail, kinds, augments)
    g2 = capi.EkfBatch(ctx, pg, 1)
    fresh = get_filter(g2, 0)
    o = oracle.Ekf(po)
    assert np.array_equal(fresh[0], np.array(o.m)) and np.array_equal(fresh[1], np.array(o.P)) and not fresh[3].any()
    for b in range(B):
        got = get_filter(g, b)
        want = fresh if b in RESET_SETS else before[b]
        for name, x, y in zip("m P Q dydx".split(), got, want):
            assert np.array_equal(x, y), (b, name)
    check_everything_but_the_filter(w, w2, snap0, kinds)
    g.close(); g2.close()


@pytest.mark.parametrize("trail", [3, 20])
def test_reset_keep_pose_equals_initialize_at_pose(oracle, ctx, trail):
    """Kind 2 in the sets 0, 2, 4: the restatement's filter is a fresh oracle filter with initializeOrientation(0) under the
    zero-vector rule and the oracle's dense transform_to(pos, q)."""
    kinds = [2, 0, 2, 0, 2]
    po, pg, g, w, w2, before, snap0 = prepared_reset(oracle, ctx, trail, kinds, seed=1)
    fresh = oracle.Ekf(po)
    for b in range(B):
        m, P, Q, dydx = get_filter(g, b)
        if b not in RESET_SETS:
            for name, x, y in zip("m P Q dydx".split(), (m, P, Q, dydx), before[b]):
                assert np.array_equal(x, y), (b, name)
            continue
        pos, q = before[b][0][POS:POS + 3], before[b][0][ORI:ORI + 4]
        e = R.reset_filter(oracle, po, True, pos, q)
        me, Pe = np.array(e.m), np.array(e.P)
        # the mean: positions are pos + 0 (exact); the orientation is four rounded products and three rounded sums of values <= 1
        assert np.array_equal(m[POS:POS + 3], pos) and np.array_equal(me[POS:POS + 3], pos)
        assert np.abs(m - me).max() <= 8 * U, (b, np.abs(m - me).max())
        assert np.abs(m[ORI:ORI + 4] - 0.5 * q).max() <= 8 * U             # the preserved quirk: q0 is not a unit quaternion
        covered = np.zeros_like(Pe, bool)
        for s, k in blocks(trail):
            blk, want = P[s:s + k, s:s + k], Pe[s:s + k, s:s + k]
            assert np.abs(blk - want).max() <= 32 * U * np.abs(want).max(), (b, s, np.abs(blk - want).max(), np.abs(want).max())
            covered[s:s + k, s:s + k] = True
        assert np.array_equal(P[~covered], Pe[~covered]) and np.array_equal(P[~covered], np.array(fresh.P)[~covered])
        assert np.array_equal(Q, np.array(fresh.Q).T.reshape(-1)) and not dydx.any()
    check_everything_but_the_filter(w, w2, snap0, kinds)
    g.close()


# ---- chain -------------------------------------------------------------------------------------------------------------------

def run_chain(oracle, ctx, trail, with_reset):
    """Filter 2 diverges (NaN mean) and only sees bad frames, its neighbours track. With resetUntilInitSucceeds the status entry
    resets it once its timer expires; three frames of imu + predict + augmentation follow. Returns the final states, the frame the
    reset fired at and the samples fed after it."""
    import torch
    rng = np.random.default_rng([trail, 99])
    po, pg = same_params(oracle, cameraTrailLength=trail)
    g = capi.EkfBatch(ctx, pg, B)
    sp = capi.session_default_params(targetFps=2.0, resetUntilInitSucceeds=int(with_reset))
    w = World(trail, 4)
    w.init_all(ctx, g, sp)
    for b in range(B):
        m, P = random_state(rng, g.n, trail, scale=1e-2)
        g.set_state(b, m, P)
    m_nan = np.full(g.n, np.nan)
    g.set_state(2, m_nan, None)
    good = np.array([1, 1, 0, 1, 1], np.uint8)
    d_good = dev(good)
    kind = torch.zeros(B, dtype=torch.int32, device="cuda")
    NS = 3
    dt_out = torch.zeros((NS, B), dtype=torch.float64, device="cuda")
    time_out = torch.zeros((NS, B), dtype=torch.float64, device="cuda")
    fired, after, fed = None, 0, []
    for f in range(20):
        t = np.repeat((0.5 * f + 0.1 * np.arange(1, NS + 1))[:, None], B, axis=1)
        gy, ac = rng.normal(0, 0.02, (NS, B, 3)), np.array([0.2, -0.1, 9.8]) + rng.normal(0, 0.05, (NS, B, 3))
        d_t, d_gy, d_ac = dev(t), dev(gy), dev(ac)
        g.session_imu_dev(w.ses, NS, d_t.data_ptr(), d_ac.data_ptr(), dt_out.data_ptr(), time_out.data_ptr())
        g.predict_n_dev(NS, dt_out.data_ptr(), d_gy.data_ptr(), d_ac.data_ptr())
        g.normalize_quaternions(True)
        g.symmetrize_augment_dev()
        if fired is not None:
            fed.append((t[:, 2].copy(), gy[:, 2].copy(), ac[:, 2].copy()))
            after += 1
            if after == 3:
                break
        g.session_status_dev(sp, w.ses, d_good.data_ptr(), kind.data_ptr())
        k = kind.cpu().tolist()
        if any(k):
            assert k == [0, 0, R.RESET_FRESH, 0, 0] and fired is None
            fired = f
            w.reset(g, sp, kind)
        elif not with_reset and f == 9:                        # the run without the reset stops where the other one does
            break
    ctx.synchronize()
    states = [g.get_state(b) for b in range(B)]
    g.close()
    return po, states, fired, fed


@pytest.mark.parametrize("trail", [3, 20])
def test_chain_diverged_filter_is_reset_and_neighbours_do_not_notice(oracle, ctx, trail):
    po, states, fired, fed = run_chain(oracle, ctx, trail, True)
    assert fired == 6 and len(fed) == 3                        # platform time 3.3 at frame 6: 0 + 3 < t for the first time
    _, plain, none_fired, _ = run_chain(oracle, ctx, trail, False)
    assert none_fired is None
    for b in (0, 1, 3, 4):
        assert np.array_equal(states[b][0], plain[b][0]) and np.array_equal(states[b][1], plain[b][1]), b
    assert np.isnan(plain[2][0]).all()                         # without the reset the diverged filter stays lost
    # the oracle's fresh filter through the same calls
    o = oracle.Ekf(po)
    first = True
    for t, gy, ac in fed:
        for s in range(len(t)):
            if first:
                o.initialize_orientation(ac[s]); first = False
            o.predict(float(t[s]), gy[s], ac[s])
        o.normalize_quaternions(1)
        o.maintain_psd()
        o.update_visual_pose_augmentation(-1)
    m, P = states[2]
    assert np.isfinite(m).all() and np.isfinite(P).all()
    assert rel(m, np.array(o.m)) <= TOL and rel(P, np.array(o.P)) <= TOL, (rel(m, np.array(o.m)), rel(P, np.array(o.P)))


# ---- capture -----------------------------------------------------------------------------------------------------------------

def test_captured_session_entries_replay_bit_equal():
    """imu + status + reset captured on a lane's stream and replayed twice from restored state: bit-equal to the eager run. Only the
    session entries are inside the captured region."""
    import torch
    trail = 3
    with capi.Lanes(1, width=64, height=64) as lanes:
        ctx = lanes.ctx[0]
        stream = torch.cuda.ExternalStream(ctx.get_stream())
        g = capi.EkfBatch(ctx, capi.ekf_default_params(cameraTrailLength=trail), B)
        sp = capi.session_default_params(targetFps=2.0, resetUntilInitSucceeds=1)
        w = World(trail, 4)
        rng = np.random.default_rng(5)
        start = [random_state(rng, g.n, trail) for _ in range(B)]
        NS = 3
        t = np.repeat((50.0 + 0.1 * np.arange(1, NS + 1))[:, None], B, axis=1)
        d_t, d_ac = dev(t), dev(np.array([0.2, -0.1, 9.8]) + rng.normal(0, 0.05, (NS, B, 3)))
        d_good = dev(np.array([1, 0, 1, 0, 0], np.uint8))
        outs = dict(dt=torch.zeros((NS, B), dtype=torch.float64, device="cuda"), time=torch.zeros((NS, B), dtype=torch.float64, device="cuda"),
                    status=torch.zeros(B, dtype=torch.int32, device="cuda"), frozen=torch.zeros(B, dtype=torch.uint8, device="cuda"),
                    kind=torch.zeros(B, dtype=torch.int32, device="cuda"))

        def restore():
            """The clock at 50 s. Sets 1 and 3: INIT with the timer expired (reset kind 1); 0 and 2: Control past INIT, the session INIT,
            the timer expired (kind 2); 4: last reset a second ago (no reset). The torch work runs on the default stream, the
            library's on the lane's: synchronised in between."""
            w.fill_sentinels(8)
            torch.cuda.synchronize()
            w.init_all(ctx, g, sp)
            for b in range(B):
                g.set_state(b, *start[b])
            ctx.synchronize()
            for k, v in (("first_sample", 0), ("first_sample_t", 10.0), ("prev_sample_t", 50.0), ("time", 40.0)):
                w.ses.m[k][:] = v
            w.ses.m["control_status"].copy_(torch.tensor([1, 0, 1, 0, 0], dtype=torch.int32))
            w.ses.m["last_reset_time"].copy_(torch.tensor([0.0, 0.0, 0.0, 0.0, 49.0], dtype=torch.float64))
            for o in outs.values():
                o.fill_(0)
            torch.cuda.synchronize()

        def frame():
            g.session_imu_dev(w.ses, NS, d_t.data_ptr(), d_ac.data_ptr(), outs["dt"].data_ptr(), outs["time"].data_ptr())
            g.session_status_dev(sp, w.ses, d_good.data_ptr(), outs["kind"].data_ptr(), status_dev=outs["status"].data_ptr(),
                                 frozen_dev=outs["frozen"].data_ptr())
            w.reset(g, sp, outs["kind"])

        def result():
            torch.cuda.synchronize()
            snap = w.snapshot()
            snap["out"] = {k: v.cpu().numpy().copy() for k, v in outs.items()}
            snap["filters"] = {b: get_filter(g, b) for b in range(B)}
            return snap

        restore()
        with torch.cuda.stream(stream):
            frame()
        eager = result()
        assert eager["out"]["kind"].tolist() == [2, 1, 2, 1, 0]
        restore()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            frame()
        for rep in range(2):
            restore()
            graph.replay()
            got = result()
            for gname in eager:
                for k in eager[gname]:
                    a, b_ = eager[gname][k], got[gname][k]
                    if isinstance(a, tuple):
                        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b_)), (rep, gname, k)
                    else:
                        assert np.array_equal(a, b_), (rep, gname, k)
        g.close()
