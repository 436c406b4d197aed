"""Guard (no GPU): every kernel-variant knob of the library, and every value of it that selects other code, is forced by at least one
GPU parity test. The knob set is parsed from the two places that define it (struct Knobs, the name table of the C ABI); the values come
from the table below; what the GPU tests force is read from their own data -- the parametrize marks and the dicts the test bodies use --
by importing the test modules (they import torch inside their functions, so this needs no GPU)."""
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hybvio_amd", "csrc")

# knob -> the non-default values that select different code (hv_internal.hpp struct Knobs says what each value does). A new knob fails
# test_every_knob_is_listed until it is listed here, and test_every_listed_value_is_forced_by_a_gpu_test until a GPU test forces it.
KNOB_VALUES = {
    "pyr_tail": [0, 1],                    # auto picks by image count
    "pyr_l0_tiled": [1],
    "gftt_tiled": [0, 1],                  # auto picks by image count
    "klt_tile": [1],
    "vu_threads": [384, 768],
    "ekf_spec_split": [1],
    "ekf_no_speculation": [1],
    "ekf_stream_gate": [0, 1],             # 0: also above 256 filters, where auto takes the streaming kernel
    "ekf_gate_kmode": [1],
    "ingest_gather": [1],
    "ekf_fused_gate": [0, 1, 2],
    "ekf_spec_mode": [3],                  # (2 is what auto runs wherever the fused gate serves the shape: no code of its own)
    "ekf_side_stream": [0, 3, 5],
    "ekf_long_fused": [0],
    "ekf_predict_chain": [0, 2],
    "ekf_short_np": [11],
    "ekf_long_first": [1, 2, 3, 4],
    "ekf_dual_update": [0],
    "ekf_visit_order": [0, 2],
    "ekf_defer_jacobian": [0],
    "ekf_split_tri": [0, 2, 3],
    "vu_tri_threads": [64, 128, 256],
    "rot_ransac_threads": [25, 256, 1024],
}
# (knob, value) -> why no GPU test forces it. Printed by the test; meant to stay empty or to hold values the source declares removed.
DELIBERATELY_UNTESTED = {}


def _knobs_of_struct():
    text = open(os.path.join(CSRC, "hv_internal.hpp")).read()
    body = re.search(r"struct Knobs \{(.*?)\n\};", text, re.S).group(1)
    return set(re.findall(r"^\s*int\s+(\w+)\s*=", body, re.M))


def _knobs_of_name_table():
    text = open(os.path.join(CSRC, "capi.hip")).read()
    body = re.search(r"KNOB_TABLE\[\]\s*=\s*\{(.*?)\n\};", text, re.S).group(1)
    entries = re.findall(r'\{"(\w+)",\s*&Knobs::(\w+)\}', body)
    assert all(name == field for name, field in entries), [e for e in entries if e[0] != e[1]]
    return {name for name, _ in entries}


def _cases(fn):
    """The parametrize marks of a test function as dicts {argument name: value}, one per case of each mark."""
    for mark in getattr(fn, "pytestmark", []):
        if mark.name != "parametrize":
            continue
        names = [n.strip() for n in mark.args[0].split(",")] if isinstance(mark.args[0], str) else list(mark.args[0])
        for case in mark.args[1]:
            values = case.values if hasattr(case, "values") else case          # pytest.param(...) or a plain value / tuple
            if len(names) == 1 and not hasattr(case, "values"):
                values = (case,)
            yield dict(zip(names, values))


def _forced_by_the_gpu_tests():
    """Every (knob, value) a GPU test forces. Per module: which parametrize argument carries which knob, and the dicts its bodies apply."""
    mods = {m: importlib.import_module(m) for m in ("test_gpu_visual_prepare", "test_gpu_large_grid", "test_gpu_lanes", "test_gpu_pyrlk",
                                                    "test_gpu_gftt", "test_gpu_ingest", "test_gpu_ekf", "test_gpu_rot_ransac")}
    variants = mods["test_gpu_visual_prepare"].VARIANTS
    by_argument = {
        "test_gpu_visual_prepare": {"variant": lambda v: variants[v]},
        "test_gpu_large_grid": {"variant": lambda v: variants[v], "threads": lambda v: {"rot_ransac_threads": v}},
        "test_gpu_rot_ransac": {"threads": lambda v: {"rot_ransac_threads": v}},
        "test_gpu_lanes": {"order": lambda v: mods["test_gpu_lanes"].LANE_ORDERS[v]},
        "test_gpu_pyrlk": {"klt_tile": lambda v: {"klt_tile": v}, "l0_tiled": lambda v: {"pyr_l0_tiled": v},
                           "tail": lambda v: {"pyr_tail": mods["test_gpu_pyrlk"].PYR_TAIL[v]}},
        "test_gpu_gftt": {"kernel": lambda v: {"gftt_tiled": mods["test_gpu_gftt"].GFTT_TILED[v]}},
        "test_gpu_ingest": {"gather": lambda v: {"ingest_gather": v}},
        "test_gpu_ekf": {"knob": lambda v: mods["test_gpu_ekf"].GATE_KNOBS[v]},
    }
    in_bodies = [mods["test_gpu_visual_prepare"].SEQUENTIAL_LOOP, mods["test_gpu_large_grid"].NO_STREAM_GATE,
                 mods["test_gpu_lanes"].LANE_DEFAULTS, {"ekf_visit_order": 2},
                 *({"ekf_predict_chain": f} for f in mods["test_gpu_ekf"].PREDICT_CHAIN_FORMS)]
    forced = set()
    for mod_name, arguments in by_argument.items():
        mod = mods[mod_name]
        assert any(getattr(m, "name", "") == "gpu" for m in [mod.pytestmark] if m is not None), mod_name
        for name, fn in vars(mod).items():
            if not (name.startswith("test_") and callable(fn)):
                continue
            for case in _cases(fn):
                for arg, to_knobs in arguments.items():
                    if arg in case:
                        forced |= set(to_knobs(case[arg]).items())
    for d in in_bodies:
        forced |= set(d.items())
    return forced


def test_the_name_table_and_the_struct_hold_the_same_knobs():
    assert _knobs_of_struct() == _knobs_of_name_table()
    assert len(_knobs_of_struct()) >= 23


def test_every_knob_is_listed():
    assert set(KNOB_VALUES) == _knobs_of_struct(), sorted(set(KNOB_VALUES) ^ _knobs_of_struct())


def test_every_listed_value_is_forced_by_a_gpu_test():
    forced = _forced_by_the_gpu_tests()
    listed = {(k, v) for k, vs in KNOB_VALUES.items() for v in vs}
    for pair, reason in sorted(DELIBERATELY_UNTESTED.items()):
        print("deliberately untested:", pair, "--", reason)
    assert set(DELIBERATELY_UNTESTED) <= listed
    assert not (set(DELIBERATELY_UNTESTED) & forced), "tested after all: drop the entry"
    missing = listed - forced - set(DELIBERATELY_UNTESTED)
    assert not missing, sorted(missing)
    unknown = {k for k, _ in forced} - set(KNOB_VALUES)
    assert not unknown, sorted(unknown)                       # a test forces a knob the library does not have


def test_the_guard_notices_a_new_knob(tmp_path, monkeypatch):
    """The parsers see a knob added to the two source tables (so test_every_knob_is_listed would fail for it)."""
    src = tmp_path / "csrc"
    src.mkdir()
    struct = open(os.path.join(CSRC, "hv_internal.hpp")).read().replace("    int vu_tri_threads = 0;", "    int new_dummy_knob = 0;\n    int vu_tri_threads = 0;", 1)
    table = open(os.path.join(CSRC, "capi.hip")).read().replace('{"vu_tri_threads", &Knobs::vu_tri_threads},',
                                                                '{"vu_tri_threads", &Knobs::vu_tri_threads}, {"new_dummy_knob", &Knobs::new_dummy_knob},', 1)
    (src / "hv_internal.hpp").write_text(struct)
    (src / "capi.hip").write_text(table)
    monkeypatch.setattr("test_knob_coverage.CSRC", str(src))
    assert _knobs_of_struct() == _knobs_of_name_table() == set(KNOB_VALUES) | {"new_dummy_knob"}
