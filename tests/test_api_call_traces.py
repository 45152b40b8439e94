"""The Python API layer asks of the context and of the library exactly what tests/golden/api_call_traces.json recorded: the same
calls, in the same order, with the same arguments (tests/api_trace_cases.py has the cases and the stand-ins; no device)."""
import json
import os

import pytest

import api_trace_cases as cases

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_call_traces.json")


@pytest.fixture(scope="module")
def golden():
    with open(_GOLDEN) as f:
        g = json.load(f)
    strings = g["strings"]
    return {name: [strings[i] for i in t] if isinstance(t, list) else t for name, t in g["traces"].items()}


def _same(name, trace, want):
    if isinstance(want, dict):
        assert cases.digest(trace) == want, name
        return
    for i, (got, exp) in enumerate(zip(trace, want)):
        assert got == exp, "%s, entry %d: %s, recorded %s (after %s)" % (name, i, got, exp, trace[max(0, i - 3):i])
    assert len(trace) == len(want), "%s: %d entries, recorded %d" % (name, len(trace), len(want))


def test_the_file_holds_every_case(golden):
    names = {"sequence:" + cases.sequence_case_name(*c) for c in cases.sequence_cases()}
    names |= {"features:" + cases.features_case_name(*c) for c in cases.features_cases()}
    assert names == set(golden) and len(names) == 360 + 192


@pytest.mark.timeout(120)
@pytest.mark.parametrize("stage", [s for s, _ in cases.STAGE_OPTIONS] + ["all/n0"])
def test_track_sequence_makes_the_recorded_calls(golden, stage):
    """every frame count and arrangement of one stage option: set-up, the two drivers, the tables' chunks, the clean-up, the downloads"""
    stage, nfeatures = (stage.split("/")[0], 0) if "/" in stage else (stage, 10)
    ran = 0
    for case in cases.sequence_cases():
        if case[:2] == (stage, nfeatures):
            name = cases.sequence_case_name(*case)
            _same(name, cases.sequence_trace(*case), golden["sequence:" + name])
            ran += 1
    assert ran == len(cases.FRAME_COUNTS) * len(cases.ARRANGEMENTS)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("stage", cases.FEATURES_STAGES)
def test_track_features_makes_the_recorded_library_calls(golden, stage):
    """three calls in a row, the third repeating its chain, in both modes, with and without guess= and age=, records mapped and copied"""
    keep, traces = [], {}
    for case in cases.features_cases():
        if case[0] == stage:
            name = cases.features_case_name(*case)
            traces[name] = cases.features_trace(*case, keep=keep)
            _same(name, traces[name], golden["features:" + name])
    assert len(traces) == 16
    if stage in cases.STAGE_ENTRY:                           # (the stand-in's slot state does make a call repeat its chain)
        assert any(cases.repeats_chain(t, cases.STAGE_ENTRY[stage]) for t in traces.values())
