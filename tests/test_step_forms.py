"""CPU test of the walk's two innermost bodies (brickmap_amd/csrc/steps.h): the move and the packed cell of the brick walk.

steps.h is plain C++ shared by the device kernels and tests/step_check.cpp, which replays the Amanatides-Woo move, the packed cell of
the brick walk with its occupancy test and field_state against a literal transcription of the reference (src/voxel.cuh:122-130,
249-258): bit-identical tmax, axis, increments, "inside", occupancy bit and state, for a few million random moves and for the edge
families a form could get wrong (ties, the 1e6 sentinel, signed zeros, binade ends, extreme tdelta, NaN, every voxel of a brick).
The same program is built and run a second time under the address and undefined-behaviour sanitizers: host code with its own main.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "step_check.cpp")


def _run(exe, rays):
    r = subprocess.run([str(exe), str(rays)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "failures 0" in r.stdout, r.stdout + r.stderr
    words = r.stdout.split()
    return int(words[1]), int(words[3]), int(words[5])


def test_step_forms_replay_reference_move(tmp_path):
    exe = tmp_path / "step_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe), SRC])
    moves, cells, states = _run(exe, 400000)
    assert moves > 4_000_000 and cells > 500_000 and states == 512  # the run did exercise the code


def test_step_forms_under_sanitizers(tmp_path):
    exe = tmp_path / "step_check_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), SRC])
    moves, cells, states = _run(exe, 40000)
    assert moves > 400_000 and cells > 500_000 and states == 512
