"""Every lowered program, byte for byte: op arrays, weight arenas, parameter index tables, arena sizes, lanes and carry tables
of the cases of tests/program_images.py against tests/golden/program_images.json, which was recorded (by
tests/golden/make_program_images.py) from the lowerings as they were before convolution launches were described by
program.Geometry.  CPU only."""
import json
import os

import pytest

import program_images

CASES = program_images.cases()


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "program_images.json")) as f:
        return json.load(f)


def test_cases_cover_the_golden_file(golden):
    assert set(golden) - {"#recorded_from"} == set(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_program_image(golden, name):
    got = CASES[name]()
    want = golden[name]
    assert {k: v for k, v in got.items() if v != want.get(k)} == {} and set(got) == set(want)
