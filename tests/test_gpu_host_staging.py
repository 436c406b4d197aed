"""The EKF's host-pointer entries stage through the arena of their context (hv_stage.hpp), which every filter batch and every other
host-pointer entry of that context shares: calls of two batches enqueued back to back, growth of the arena behind an entry that returned
before its kernel ran, and the hybrid visit's own apply mask. Every expectation is byte equality with a sequence that cannot collide."""
import ctypes as C

import numpy as np
import pytest

from hybvio_amd import capi, synth
from hybvio_amd.capi import f64p, i32p, u8p

pytestmark = pytest.mark.gpu


def _context():
    return capi.Context(width=64, height=64, levels=1, pool_size=1)


def _spd_states(rng, B, n, scale=1e-4):
    m = rng.normal(size=(B, n))
    P = np.zeros((B, n, n))
    for b in range(B):
        A = rng.normal(size=(n, n)) * 1e-3
        P[b] = np.eye(n) * scale + A @ A.T
    return m, P


def _set(g, m, P):
    for b in range(g.batch):
        g.set_state(b, m[b], P[b])


def _states(g):
    return [g.get_state(b) for b in range(g.batch)]


def _same(a, b):
    return all(np.array_equal(ma, mb) and np.array_equal(Pa, Pb) for (ma, Pa), (mb, Pb) in zip(a, b))


class _Raw:
    """The entries as the C ABI has them: no synchronise behind a call (capi.EkfBatch adds one). Host arrays stay referenced until
    the caller has synchronised."""

    def __init__(self, g):
        self.g, self.keep = g, []

    def _a(self, a, dt):
        a = np.ascontiguousarray(a, dt)
        self.keep.append(a)
        return a

    def _H(self, H):                                                # [batch][rows][cols] -> column-major per filter
        return self._a(np.transpose(np.asarray(H, np.float64), (0, 2, 1)), np.float64)

    def _chk(self, rc):
        assert rc == 0, capi.lib().hv_status_string(rc).decode()

    def predict_n(self, dt, gyro, acc):
        dt, gyro, acc = self._a(dt, np.float64), self._a(gyro, np.float64), self._a(acc, np.float64)
        self._chk(capi.lib().hv_ekf_predict_n(self.g._h, dt.shape[0], dt.ctypes.data_as(f64p), gyro.ctypes.data_as(f64p), acc.ctypes.data_as(f64p)))

    def update(self, H, y, r_diag, active=None):
        nr, l = H.shape[1:]
        Hc, y, rd = self._H(H), self._a(y, np.float64), self._a(r_diag, np.float64)
        act = self._a(active, np.uint8) if active is not None else None
        self._chk(capi.lib().hv_ekf_update(self.g._h, nr, l, Hc.ctypes.data_as(f64p), y.ctypes.data_as(f64p), rd.ctypes.data_as(f64p),
                                           act.ctypes.data_as(u8p) if act is not None else None, 0))

    def visual_update(self, H, v, r, active=None):
        nr, l = H.shape[1:]
        Hc, v = self._H(H), self._a(v, np.float64)
        act = self._a(active, np.uint8) if active is not None else None
        self._chk(capi.lib().hv_ekf_visual_update(self.g._h, nr, l, Hc.ctypes.data_as(f64p), v.ctypes.data_as(f64p), r,
                                                  act.ctypes.data_as(u8p) if act is not None else None))

    def augment(self, discarded, active):
        d, act = self._a(discarded, np.int32), self._a(active, np.uint8)
        self._chk(capi.lib().hv_ekf_augment(self.g._h, d.ctypes.data_as(i32p), act.ctypes.data_as(u8p)))

    def undo_augment(self, active):
        act = self._a(active, np.uint8)
        self._chk(capi.lib().hv_ekf_undo_augment(self.g._h, act.ctypes.data_as(u8p)))


def test_two_filter_batches_share_one_arena():
    """Two batches of 3 filters (trail 1) on ONE context, five host-pointer calls alternating between them with no synchronise in
    between -- predict_n (3 samples), update (2 rows, flags with one zero), visual_update (4 rows), augment (discarded slots and flags),
    undo_augment (flags): each call's staged inputs sit in the shared arena until its kernel has read them, and the next call writes
    the same bytes. Both batches end byte-identical to the same calls with each batch on a context of its own."""
    rng = np.random.default_rng(20251)
    B, par = 3, capi.ekf_default_params(cameraTrailLength=1)
    n = 20 + 7 * 1                                                  # one trail pose behind the 20 inertial states
    _, PA = _spd_states(rng, B, n)
    _, PB = _spd_states(rng, B, n)
    mA, mB = (synth.visual_tracks(rng, B, 1, 2, False)[2] for _ in range(2))     # means with unit quaternions
    dt = np.full((3, B), 0.005); gyro = 0.1 * rng.normal(size=(3, B, 3)); acc = np.array([0, 0, 9.8]) + 0.1 * rng.normal(size=(3, B, 3))
    Hu, yu, ru = rng.normal(size=(B, 2, n)), 0.01 * rng.normal(size=(B, 2)), np.full(B, 1e-2)
    Hv, vv = rng.normal(size=(B, 4, n)), 0.01 * rng.normal(size=(B, 4))
    mask_u, mask_a, mask_d = np.array([1, 0, 1], np.uint8), np.array([1, 1, 0], np.uint8), np.array([0, 1, 1], np.uint8)
    dropped = np.zeros(B, np.int32)

    def calls_a(a):
        return [lambda: a.predict_n(dt, gyro, acc), lambda: a.visual_update(Hv, vv, 0.05), lambda: a.undo_augment(mask_d)]

    def calls_b(b):
        return [lambda: b.update(Hu, yu, ru, mask_u), lambda: b.augment(dropped, mask_a)]

    with _context() as ctx:
        gA, gB = capi.EkfBatch(ctx, par, B), capi.EkfBatch(ctx, par, B)
        assert gA.n == n
        _set(gA, mA, PA); _set(gB, mB, PB)
        a, b = _Raw(gA), _Raw(gB)
        ca, cb = calls_a(a), calls_b(b)
        ca[0](); cb[0](); ca[1](); cb[1](); ca[2]()                 # A.predict_n, B.update, A.visual_update, B.augment, A.undo_augment
        ctx.synchronize()
        shared = _states(gA), _states(gB)
        gA.close(); gB.close()
    alone = []
    for m, P, calls in ((mA, PA, calls_a), (mB, PB, calls_b)):
        with _context() as ctx:
            g = capi.EkfBatch(ctx, par, B)
            _set(g, m, P)
            raw = _Raw(g)
            for call in calls(raw):
                call()
            ctx.synchronize()
            alone.append(_states(g))
            g.close()
    assert not _same(shared[0], [(mA[b], PA[b]) for b in range(B)]) and not _same(shared[1], [(mB[b], PB[b]) for b in range(B)])
    assert _same(shared[0], alone[0]) and _same(shared[1], alone[1])


def test_arena_growth_behind_an_asynchronous_update():
    """One batch of 8 filters, trail 20 (n = 20 + 7 * 20 = 160, every column of the state): hv_ekf_update with 1 row and 1 column,
    then at once with 48 rows and 160 columns. hv_create has reserved the arena for hv_klt_track at max_tracks = 200 (4 208 bytes),
    hv_ekf_create for the batch's small sections -- residuals 160 x 8 doubles, IMU samples 7 x 32 x 8 doubles, two [8] double, two
    [8] int and one [8] byte vector, each padded to 16 bytes: 24 784 bytes; the second Jacobian alone is 48 x 160 x 8 doubles =
    491 520 bytes, so the second call frees and reallocates the arena while the first call's kernel may not have run. Growth
    drains the stream first: the states are byte-identical to the same two calls on a context whose arena a throw-away 48 x 160
    gate has grown, with a synchronise between."""
    rng = np.random.default_rng(20252)
    B, par = 8, capi.ekf_default_params(cameraTrailLength=20)
    n = 160
    m, P = _spd_states(rng, B, n)
    H1, y1 = rng.normal(size=(B, 1, 1)), 0.01 * rng.normal(size=(B, 1))
    H2, y2 = rng.normal(size=(B, 48, n)), 0.01 * rng.normal(size=(B, 48))
    r = np.full(B, 1e-2)
    with _context() as ctx:
        g = capi.EkfBatch(ctx, par, B)
        assert g.n == n
        _set(g, m, P)
        raw = _Raw(g)
        raw.update(H1, y1, r)
        raw.update(H2, y2, r)
        ctx.synchronize()
        grown = _states(g)
        g.close()
    with _context() as ctx:
        g = capi.EkfBatch(ctx, par, B)
        _set(g, m, P)
        g.visual_gate(H2, y2, 1.0)                                  # (a gate changes no state)
        raw = _Raw(g)
        raw.update(H1, y1, r)
        ctx.synchronize()
        raw.update(H2, y2, r)
        ctx.synchronize()
        calm = _states(g)
        g.close()
    assert not _same(grown, [(m[b], P[b]) for b in range(B)])
    assert _same(grown, calm)


def test_hybrid_visit_keeps_its_apply_mask_to_itself():
    """hv_ekf_visual_track_hybrid directly behind an hv_ekf_update whose flags switch off a filter the visit applies (two poses, two
    cameras, hybridMapSize 1): the visit's apply mask is a buffer of its own, so the result equals the visit alone from the state the
    update left."""
    rng = np.random.default_rng(20253)
    B, trail_len, M, npose = 6, 1, 1, 2
    T1, T2, means, idx, feat = synth.visual_tracks(rng, B, trail_len, npose, True)
    vel = 0.2 * rng.normal(size=feat.shape)
    n = means.shape[1] + 3 * M
    m0 = np.concatenate([means, rng.normal(size=(B, 3 * M))], axis=1)
    _, P0 = _spd_states(rng, B, n)
    ys = feat.reshape(B, -1) + 2e-3 * rng.normal(size=(B, feat.shape[1] * 2))
    vp = capi.vu_default_params(imu_to_camera=T1, second_imu_to_camera=T2)
    par = capi.ekf_default_params(cameraTrailLength=trail_len, hybridMapSize=M)
    Hu = np.zeros((B, 2, n)); Hu[:, 0, 0] = 1.0; Hu[:, 1, 4] = 1.0
    yu, ru = 1e-3 * rng.normal(size=(B, 2)), np.full(B, 1e-2)
    flags = np.array([1, 0, 0, 0, 1, 0], np.uint8)
    idx32, none = np.ascontiguousarray(idx, np.int32), np.full(B, -1, np.int32)
    vptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def hybrid(g):
        st, gs = np.full((B, 2), -9, np.int32), np.full(B, -9, np.int32)
        chi, pf = np.zeros(B), np.zeros((B, 3))
        rc = capi.lib().hv_ekf_visual_track_hybrid(g._h, C.byref(vp), npose, vptr(idx32), vptr(feat), vptr(vel), vptr(ys), vptr(none), vptr(none),
                                                   1.5, 0.05, vptr(st), vptr(gs), vptr(chi), vptr(pf))
        assert rc == 0, capi.lib().hv_status_string(rc).decode()
        return st, gs, chi, pf, _states(g)

    feat, vel, ys = (np.ascontiguousarray(a, np.float64) for a in (feat, vel, ys))
    with _context() as ctx:
        g = capi.EkfBatch(ctx, par, B)
        assert g.n == n
        _set(g, m0, P0)
        raw = _Raw(g)
        raw.update(Hu, yu, ru, flags)
        behind = hybrid(g)
        g.close()
    with _context() as ctx:
        g = capi.EkfBatch(ctx, par, B)
        _set(g, m0, P0)
        g.update(Hu, yu, ru, flags)                                 # (synchronises)
        left = _states(g)
        g.close()
    with _context() as ctx:
        g = capi.EkfBatch(ctx, par, B)
        _set(g, [s[0] for s in left], [s[1] for s in left])
        alone = hybrid(g)
        g.close()
    applied_off = [k for k in range(B) if not flags[k] and behind[1][k] == 0 and not np.array_equal(behind[4][k][1], left[k][1])]
    assert applied_off, behind[1]                                   # the visit applied the track of a filter the update had switched off
    for x, y in zip(behind[:4], alone[:4]):
        assert np.array_equal(x, y)
    assert _same(behind[4], alone[4])
