"""The argument errors of the package's Python layer, replayed against tests/golden/api_errors.json (written by
tests/golden/make_api_errors.py): every case raises the recorded exception type with the recorded text, so a function keeps
finding the same argument first and saying the same thing about it.  No GPU needed: tests/api_error_cases.py says how."""
import json
import os

import pytest

import api_error_cases

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "api_errors.json")) as f:
    RECORDED = json.load(f)


@pytest.fixture(scope="module")
def cases():
    return dict(api_error_cases.cases())


def test_the_list_and_the_record_name_the_same_cases(cases):
    assert sorted(cases) == sorted(RECORDED)
    assert len(cases) >= 400


def test_every_case_raises_what_was_recorded(cases):
    wrong = []
    for name, fn in cases.items():
        got = api_error_cases.record(fn)
        want = (RECORDED[name]["type"], RECORDED[name]["message"])
        if got != want:
            wrong.append((name, got, want))
    assert not wrong, wrong[:10]


def test_the_record_reaches_every_kind_of_check():
    """Not a tensor or array, wrong dtype, wrong shape or element count, not contiguous, on the CPU, and the scalar ranges."""
    text = " | ".join(r["message"] for r in RECORDED.values())
    for words in ("must be a torch tensor", "must be a numpy array", "has dtype", "has shape", "must be contiguous", "is on cpu; expected cuda:0",
                  "is on cpu; expected a cuda device", "iterations is", "sigma_c is", "sigma_n is", "sigma_p is", "max_history is", "spp is",
                  "num_parts must be 1", "render_adaptive needs", "is not a camera field", "is not a shading field", "must be a pinhole",
                  "needs a pinhole camera", "must be a Camera", "bad render parameters", "hits must be a 4-byte"):
        assert words in text, words
    assert {r["type"] for r in RECORDED.values()} >= {"ValueError", "MirtError"}
