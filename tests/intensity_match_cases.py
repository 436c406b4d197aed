"""The fixtures of the intensity-matching tests and what the restatement makes of them (not collected; imported by
test_intensity_match_restatement.py, which checks the rounding-boundary condition on every one of them, and by
test_gpu_intensity_match.py, which runs them on the device).

Frames are crops of hybvio_amd.synth.stereo_sequence(11, 752, 480, 4): set s takes its own crop, frame f a brightness drift of its own
(so the successive step has something to do), the right image one of three gain / offset pairs. A case is a small record; expected()
runs tests/intensity_match_restatement.py over it once and is cached."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import intensity_match_restatement as R
from hybvio_amd import synth

GAINS = ((0.8, 12.0), (1.25, -20.0), (0.55, 40.0))                           # of the right image, by set
DRIFT = ((1.0, 0.0), (0.9, 10.0), (1.1, -8.0), (0.95, 5.0))                  # of both images, by frame


@dataclasses.dataclass(frozen=True)
class Case:
    h: int
    w: int
    stride: int                      # row stride in bytes of the device buffers
    sets: int
    frames: int
    successive: float                # matchSuccessiveIntensities
    stereo: bool                     # matchStereoIntensities
    mono: bool = False               # right_dev = NULL
    kind: str = "crops"              # crops | clamp | special | one_pixel
    inactive: tuple = ()             # sets masked out by active_dev


CASES = {
    "480x752_both": Case(480, 752, 752, 3, 2, 0.5, True),
    "sets67": Case(33, 47, 48, 67, 2, 0.5, True),
    "sets1": Case(33, 47, 48, 1, 2, 0.5, True),
    "mask": Case(33, 47, 48, 7, 2, 0.5, True, inactive=(0, 3, 6)),
    "recursion_w025": Case(97, 131, 144, 3, 4, 0.25, True),
    "recursion_w1": Case(97, 131, 144, 3, 4, 1.0, True),
    "clamp": Case(33, 47, 50, 3, 1, 0.0, True, kind="clamp"),
    "special": Case(5, 7, 16, 3, 2, 0.5, True, kind="special"),
    "one_pixel": Case(1, 1, 1, 2, 2, 0.5, True, kind="one_pixel"),
}
# stride: 97 x 131 rounded up past the width; 33 x 47 with rows that are not 16-byte aligned; 5 x 7 dense
for _h, _w, _stride in ((97, 131, 144), (33, 47, 50), (5, 7, 7)):
    CASES[f"{_h}x{_w}_stereo"] = Case(_h, _w, _stride, 3, 2, 0.0, True)
    CASES[f"{_h}x{_w}_successive_mono"] = Case(_h, _w, _stride, 3, 2, 0.25, False, mono=True)
    CASES[f"{_h}x{_w}_both"] = Case(_h, _w, _stride, 3, 2, 0.5, True)


def gain(img, g, o):
    return np.clip(np.rint(img.astype(np.float64) * g + o), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _base():
    left, right, _ = synth.stereo_sequence(11, 752, 480, 4)
    return left, right


def crop(img, s, h, w):
    y0, x0 = (37 * s) % (img.shape[0] - h + 1), (53 * s) % (img.shape[1] - w + 1)
    return img[y0:y0 + h, x0:x0 + w]


@functools.lru_cache(maxsize=None)
def frames(name):
    """[(left [sets, h, w], right [sets, h, w]), ...] per frame; uint8."""
    c = CASES[name]
    left, right = _base()
    out = []
    for f in range(c.frames):
        L = np.empty((c.sets, c.h, c.w), np.uint8)
        Rt = np.empty_like(L)
        for s in range(c.sets):
            l, r = crop(left[f], s, c.h, c.w), crop(right[f], s, c.h, c.w)
            if c.kind == "clamp":
                # a left frame stretched until it saturates at both ends: its standard deviation pushes the flat right frame's
                # table, and pixels, past 0 and past 255
                l, r = gain(l, 3.0, -256.0), gain(r, *GAINS[2])
            elif c.kind == "special":
                two = np.where(l > np.median(l), 200, 10).astype(np.uint8)
                other = np.where(r > np.median(r), 90 + f, 60).astype(np.uint8)
                l, r = ((np.full_like(l, 255), two), (two, np.full_like(l, 255)), (two, other))[s]
            elif c.kind == "one_pixel":
                l, r = l[:1, :1], r[:1, :1]
            else:
                l, r = gain(l, *DRIFT[f]), gain(gain(r, *DRIFT[f]), *GAINS[s % 3])
            L[s], Rt[s] = l, r
        out.append((L, Rt))
    return out


@dataclasses.dataclass
class Expected:
    left: np.ndarray                 # [sets, h, w] after the frame
    right: np.ndarray
    records: list                    # R.Record per set (None: inactive)
    prev_sum: list
    prev_sqsum: list
    has_prev: list


@functools.lru_cache(maxsize=None)
def expected(name):
    """Per frame what the device must leave behind; inactive sets keep pixels and state."""
    c = CASES[name]
    seqs = [R.Sequence() for _ in range(c.sets)]
    out = []
    for L, Rt in frames(name):
        eL, eR, recs = L.copy(), Rt.copy(), []
        for s in range(c.sets):
            if s in c.inactive:
                recs.append(None)
                continue
            l, r, rec = seqs[s].frame(L[s], None if c.mono else Rt[s], c.successive, c.stereo)
            eL[s] = l
            if r is not None:
                eR[s] = r
            recs.append(rec)
        out.append(Expected(eL, eR, recs, [q.prev_sum for q in seqs], [q.prev_sqsum for q in seqs], [q.has_prev for q in seqs]))
    return out


def min_boundary_distance(name) -> float:
    """Smallest distance of an in-range table entry of the case from a rounding boundary."""
    d = np.inf
    for e in expected(name):
        for rec in e.records:
            if rec is not None:
                d = min([d] + [R.boundary_distance(v) for v in rec.v if v is not None])
    return d


HOST_WEIGHTS = (1.0, 0.25)


def host_pairs():
    """(l, r, weight) of the one-pair entries: 97 x 131, the first two sets of the stereo case."""
    L, Rt = frames("97x131_stereo")[0]
    return [(L[i], Rt[i], w) for i, w in enumerate(HOST_WEIGHTS)]
