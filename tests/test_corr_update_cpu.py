"""The update rule of the matching-cost factors (csrc/gp_corr_update.hpp: which pose the stored correspondences belong to; keep / stored / note a linearise) against
an f64 restatement of the reference's update_correspondences decision (tests/icp_ref.py: ICPFactorRef.keeps_correspondences, integrated_icp_factor_impl.hpp
:129-137; the LOAM and colored GICP factors state the same rule), without a device and without loading anything into Python: tests/corr_update_cases.cpp includes
the header alone, is built with the host compiler under AddressSanitizer and UBSan, and runs as a plain program over the cases below.

The poses of the cases are chosen so that both sides compute the pose difference exactly (identity or quarter / half turns about z, dyadic translations): a
tolerance "equal to the difference" is then equal for both, and one ulp decides."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import icp_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gtsam_points_amd", "csrc")


def pose(turns_z=0.0, t=(0.0, 0.0, 0.0)):
    """a rotation by turns_z quarter turns about z (exact entries) and a translation"""
    c, s = {0: (1.0, 0.0), 1: (0.0, 1.0), 2: (-1.0, 0.0), 3: (0.0, -1.0)}[int(turns_z) % 4]
    T = np.eye(4)
    T[:3, :3] = [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = t
    return T


A = pose(0, (1.0, 2.0, 3.0))
NEAR = pose(0, (1.5, 2.0, 3.0))     # |t| differs from A by exactly 0.5, no rotation
QUARTER = pose(1, (1.0, 2.0, 3.0))  # rotation differs from A by exactly atan2(1, 0), the same origin... (R^T (t_A - t_Q) = 0)
HALF = pose(2, (1.0, 2.0, 3.0))     # a rotation by pi
FAR = pose(1, (40.0, -7.0, 3.0))
UP = lambda x: math.nextafter(x, math.inf)  # noqa: E731

# (name, [("T", rot, trans) | ("L", pose) | ("E", pose)])
CASES = [
    ("no stored correspondences", [("T", 1.0, 1.0), ("L", A)]),
    ("no stored correspondences: error first", [("T", 1.0, 1.0), ("E", A), ("E", A), ("L", A)]),
    ("both tolerances zero", [("L", A), ("L", A), ("E", A)]),
    ("only the rotation tolerance positive", [("T", 1.0, 0.0), ("L", A), ("L", A), ("L", NEAR)]),
    ("only the translation tolerance positive", [("T", 0.0, 1.0), ("L", A), ("L", A), ("L", NEAR)]),
    ("translation equal to its tolerance", [("T", 1.0, 0.5), ("L", A), ("L", NEAR)]),
    ("translation one ulp below its tolerance", [("T", 1.0, UP(0.5)), ("L", A), ("L", NEAR)]),
    ("rotation equal to its tolerance", [("T", math.atan2(1.0, 0.0), 1.0), ("L", A), ("L", QUARTER)]),
    ("rotation one ulp below its tolerance", [("T", UP(math.atan2(1.0, 0.0)), 1.0), ("L", A), ("L", QUARTER)]),
    ("a rotation by pi", [("T", 3.0, 1.0), ("L", A), ("L", HALF), ("T", 4.0, 1.0), ("L", A)]),
    ("pose_lin is the last linearisation pose, not the search pose", [("T", 1.0, 1.0), ("L", A), ("L", NEAR), ("E", NEAR)]),
    ("pose_lin is the search pose after a later kept linearise", [("T", 1.0, 1.0), ("L", A), ("L", NEAR), ("E", A), ("E", NEAR)]),
    ("a foreign pose_lin", [("T", 1.0, 1.0), ("L", A), ("L", NEAR), ("E", FAR), ("E", NEAR), ("E", FAR), ("L", FAR), ("L", A)]),
    ("the scripted sequence of the digest", [("T", 0.1, 1.0), ("L", A), ("L", NEAR), ("E", NEAR), ("E", A), ("E", FAR), ("L", pose(3, (-9.0, 0.0, 0.0)))]),
]


class RuleRef:
    """The reference's rule on icp_ref.ICPFactorRef's own fields and decision, plus what the C layer adds for error(): the stored correspondences serve pose_lin when
    it is the pose of the last linearise or the pose they were searched at; a search for an error evaluation leaves no linearise behind it."""

    def __init__(self):
        self.ref = icp_ref.ICPFactorRef(np.zeros((1, 3)), np.zeros((1, 3)))
        self.lin = None

    def search(self, p):
        self.ref.correspondences = True  # (any: the decision only asks whether some are stored)
        self.ref.last_correspondence_point = np.array(p)
        self.lin = None

    def linearize(self, p):
        keep = self.ref.keeps_correspondences(p)
        if not keep:
            self.search(p)
        self.lin = np.array(p)
        return f"L keep={int(keep)}"

    def error(self, p):
        stored = self.ref.correspondences is not None and ((self.lin is not None and np.array_equal(self.lin, p)) or np.array_equal(self.ref.last_correspondence_point, p))
        if not stored:
            self.search(p)
        return f"E stored={int(stored)} lin_valid={int(self.lin is not None)}"


def _line(op):
    if op[0] == "T":
        return f"T {float(op[1]).hex()} {float(op[2]).hex()}"
    return op[0] + " " + " ".join(float(x).hex() for x in np.asarray(op[1], dtype=np.float64).T.reshape(16))  # column-major


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("corr_update") / "corr_update_cases")
    # the host compiler alone: no hipcc, no HIP include path -- the header must stand without them
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "corr_update_cases.cpp"), "-o", exe])
    return exe


def test_update_rule_matches_the_reference_decision(program, tmp_path):
    script, want = [], []
    for name, ops in CASES:
        script.append("N " + name)
        want.append("N " + name)
        rule = RuleRef()
        for op in ops:
            script.append(_line(op))
            if op[0] == "T":
                rule.ref.set_correspondence_update_tolerance(op[1], op[2])
            else:
                want.append(rule.linearize(op[1]) if op[0] == "L" else rule.error(op[1]))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(script) + "\n")
    run = subprocess.run([program, str(path)], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr  # (a sanitizer report goes to stderr and fails the run)
    got = run.stdout.splitlines()
    assert got == want, "\n".join(f"{g!r:60} {w!r}" for g, w in zip(got, want))


def test_the_cases_decide_what_their_names_say():
    """the restatement's own answers at the cases' edges, so that a case cannot pass by both sides missing its point"""
    def run(ops):
        rule, out = RuleRef(), []
        for op in ops:
            if op[0] == "T":
                rule.ref.set_correspondence_update_tolerance(op[1], op[2])
            else:
                out.append(rule.linearize(op[1]) if op[0] == "L" else rule.error(op[1]))
        return out

    by = {name: run(ops) for name, ops in CASES}
    assert icp_ref.pose_difference(NEAR, A) == (0.0, 0.5) and icp_ref.pose_difference(QUARTER, A) == (math.atan2(1.0, 0.0), 0.0)
    assert icp_ref.pose_difference(HALF, A)[0] == math.pi
    assert by["no stored correspondences"] == ["L keep=0"]
    assert by["both tolerances zero"] == ["L keep=0", "L keep=0", "E stored=1 lin_valid=1"]
    assert by["only the rotation tolerance positive"] == by["only the translation tolerance positive"] == ["L keep=0"] * 3  # (both comparisons are strict: 0 < 0 fails)
    assert by["translation equal to its tolerance"][-1] == "L keep=0" and by["translation one ulp below its tolerance"][-1] == "L keep=1"
    assert by["rotation equal to its tolerance"][-1] == "L keep=0" and by["rotation one ulp below its tolerance"][-1] == "L keep=1"
    assert by["a rotation by pi"] == ["L keep=0", "L keep=0", "L keep=1"]  # pi < 3 fails, pi < 4 holds
    assert by["pose_lin is the last linearisation pose, not the search pose"] == ["L keep=0", "L keep=1", "E stored=1 lin_valid=1"]
    assert by["pose_lin is the search pose after a later kept linearise"][-2:] == ["E stored=1 lin_valid=1"] * 2
    assert by["a foreign pose_lin"][2:5] == ["E stored=0 lin_valid=0", "E stored=0 lin_valid=0", "E stored=0 lin_valid=0"]
