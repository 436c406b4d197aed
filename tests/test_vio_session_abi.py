"""CPU checks of hv_vio_create_session (added within ABI 4): the symbol, the defaults of the members it alone reads member for member
against their own default functions, the member order of hv_vio_params and hv_vio_view against the header, and every decision it
takes before the context is looked at (made with a NULL context, which is itself the last refusal: an accepted parameter set
returns HV_ERR_INVALID, one that is left out HV_ERR_UNSUPPORTED)."""
import ctypes as C
import os
import re

from hybvio_amd import capi

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "hybvio_hip.h")
INVALID, UNSUPPORTED = -1, -2
MONO = dict(trail__useStereo=0, output__useStereo=0)


def _create(p, n_sets=2, out=True, ctx=None, name="hv_vio_create_session"):
    h = C.c_void_p()
    return getattr(capi.lib(), name)(ctx, C.byref(p) if p is not None else None, n_sets, C.byref(h) if out else None)


def test_symbol_and_unchanged_abi():
    L = capi.lib()
    text = open(HEADER).read()
    assert hasattr(L, "hv_vio_create_session") and "hv_vio_create_session" in capi.PROTOTYPES
    assert re.search(r"\bhv_vio_create_session\(", text)
    assert L.hv_abi_version() == 4 and "HV_K_COUNT = 20 }" in text
    assert L.hv_vio_frame(None, 16, None, 64, 8, 1, 16, 16, 16) == INVALID


def test_new_defaults_are_those_of_the_owned_entries_member_for_member():
    L = capi.lib()
    p = capi.vio_default_params()
    own = dict(ransac5=(capi.Ransac5Params, "hv_ransac5_default_params"), upright2p=(capi.Upright2pParams, "hv_upright2p_default_params"),
               fast=(capi.FastParams, "hv_fast_default_params"), gftt_legacy=(capi.GfttLegacyParams, "hv_gftt_legacy_default_params"))
    for member, (cls, fn) in own.items():
        d = cls()
        getattr(L, fn)(C.byref(d))
        got = getattr(p, member)
        assert len(cls._fields_) > 0
        for name, _ in cls._fields_:
            assert getattr(got, name) == getattr(d, name), (member, name)
    assert (p.useStereoUpright2p, p.useHybridRansac) == (0, 1)
    # the defaults that existed stay
    assert (p.featureDetector, p.useRansac3, p.predictOpticalFlow, p.batchVisualUpdate) == (capi.DETECTOR_GPU_GFTT, 1, 1, 0)
    assert (p.ransacRngSeed, p.odometryRngSeed, p.imu_samples_max) == (4649, 0, 32)
    # an override reaches the new members
    q = capi.vio_default_params(ransac5__ransac2InliersToSkipRansac5=2.0, fast__maxTracks=120, useHybridRansac=0)
    assert (q.ransac5.ransac2InliersToSkipRansac5, q.fast.maxTracks, q.useHybridRansac) == (2.0, 120, 0)


def test_new_members_are_appended_in_the_header_order():
    text = open(HEADER).read()
    body = re.search(r"typedef struct hv_vio_params \{(.*?)\} hv_vio_params;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") if decl.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    fields = [k for k, _ in capi.VioParams._fields_]
    assert names == fields
    assert fields[-6:] == ["ransac5", "upright2p", "fast", "gftt_legacy", "useStereoUpright2p", "useHybridRansac"]
    assert [k for k, _ in capi.VioView._fields_][-3:] == ["ransac_result", "ransac_score", "r5_summary"]
    view = re.search(r"typedef struct hv_vio_view \{(.*?)\} hv_vio_view;", text, re.S).group(1)
    assert view.index("slot_right") < view.index("*ransac_result") < view.index("*ransac_score") < view.index("*r5_summary")


def test_sessions_accepted_up_to_the_null_context():
    ok = capi.vio_default_params
    accepted = (dict(),                                                       # the default session
                MONO,
                dict(featureDetector=capi.DETECTOR_FAST), dict(featureDetector=capi.DETECTOR_GFTT),
                dict(useRansac3=0, useStereoUpright2p=1),
                dict(useRansac3=0, useStereoUpright2p=1, useHybridRansac=0),
                dict(useRansac3=0, useHybridRansac=1),
                dict(useRansac3=0, useStereoUpright2p=0, useHybridRansac=0),
                dict(MONO, useStereoUpright2p=1),                             # falls through to hybrid: two cameras are needed
                dict(MONO, useRansac3=0, useHybridRansac=0),
                dict(MONO, featureDetector=capi.DETECTOR_FAST), dict(MONO, featureDetector=capi.DETECTOR_GFTT),
                # the draw counts of filters that are not selected are not looked at
                dict(MONO, ransac3__ransac3MaxIterations=capi.RNG_MAX_DRAWS),
                dict(upright2p__ransacStereoUpright2pMaxIterations=capi.RNG_MAX_DRAWS),
                dict(useRansac3=0, ransac3__ransac3MaxIterations=capi.RNG_MAX_DRAWS),
                dict(useRansac3=0, useStereoUpright2p=1, upright2p__ransacStereoUpright2pMaxIterations=capi.RNG_MAX_DRAWS // 2))
    for over in accepted:
        assert _create(ok(**over)) == INVALID, over
    assert _create(ok(**MONO), n_sets=65535) == INVALID
    # a consistent non-default size with each detector
    size = dict(tracks__maxTracks=120, trail__maxTracks=120, gftt__maxTracks=120, output__maxTracks=120)
    assert _create(ok(**size)) == INVALID
    assert _create(ok(**size, featureDetector=capi.DETECTOR_FAST, fast__maxTracks=120)) == INVALID
    assert _create(ok(**size, featureDetector=capi.DETECTOR_GFTT, gftt_legacy__maxTracks=120)) == INVALID


def test_what_is_still_left_out_is_unsupported():
    ok = capi.vio_default_params
    left_out = (dict(gate__independentStereoOpticalFlow=1), dict(predictOpticalFlow=0), dict(batchVisualUpdate=1), dict(trail__fullPointCloud=1),
                dict(ekf__hybridMapSize=4), dict(ransac3__ransac3MaxIterations=capi.RNG_MAX_DRAWS),
                dict(useRansac3=0, useStereoUpright2p=1, upright2p__ransacStereoUpright2pMaxIterations=capi.RNG_MAX_DRAWS // 2 + 1))
    for bad in left_out:
        assert _create(ok(**bad)) == UNSUPPORTED, bad
        for more in (MONO, dict(featureDetector=capi.DETECTOR_FAST), dict(useRansac3=0)):
            if not any("Iterations" in k for k in bad):                          # (the draw counts belong to one filter each)
                assert _create(ok(**bad, **more)) == UNSUPPORTED, (bad, more)
    assert _create(ok(), n_sets=65536) == UNSUPPORTED and _create(ok(**MONO), n_sets=65536) == UNSUPPORTED
    # hv_vio_create refuses the same and, as before, every session but the default one
    for bad in left_out[:5] + (MONO, dict(featureDetector=capi.DETECTOR_FAST), dict(useRansac3=0)):
        assert _create(ok(**bad), name="hv_vio_create") == UNSUPPORTED, bad
    # ... and does not read the new members
    assert _create(ok(useStereoUpright2p=1, useHybridRansac=0, fast__maxTracks=7, gftt_legacy__maxTracks=7), name="hv_vio_create") == INVALID


def test_invalid_arguments_come_first():
    ok = capi.vio_default_params
    assert _create(None) == INVALID and _create(ok(), out=False) == INVALID
    assert _create(ok(), n_sets=0) == INVALID and _create(ok(), n_sets=-1) == INVALID
    for bad in (dict(imu_samples_max=0), dict(imu_samples_max=33), dict(tracks__maxTracks=100), dict(trail__maxTracks=100),
                dict(gftt__maxTracks=100), dict(output__maxTracks=100), dict(ekf__cameraTrailLength=10), dict(output__cameraTrailLength=10),
                dict(output__maxVisualUpdates=10), dict(output__maxSuccessfulVisualUpdates=3),
                dict(trail__useStereo=0), dict(output__useStereo=0),           # the index and the output disagree about stereo
                dict(session__visualUpdateForEveryNFrame=0),
                dict(featureDetector=capi.DETECTOR_FAST, fast__maxTracks=100),  # the selected detector's maxTracks
                dict(featureDetector=capi.DETECTOR_GFTT, gftt_legacy__maxTracks=100),
                dict(featureDetector=3), dict(featureDetector=-1)):
        assert _create(ok(**bad)) == INVALID, bad
        # an invalid argument is reported before an unsupported one
        assert _create(ok(**bad, batchVisualUpdate=1, ekf__hybridMapSize=4)) == INVALID, bad
        assert _create(ok(**bad), n_sets=65536) == INVALID, bad
    # the maxTracks of a detector that is not selected is not looked at (gftt's is one of hv_vio_create's own checks)
    assert _create(ok(fast__maxTracks=100, gftt_legacy__maxTracks=100)) == INVALID
    assert _create(ok(fast__maxTracks=100, gftt_legacy__maxTracks=100, batchVisualUpdate=1)) == UNSUPPORTED
