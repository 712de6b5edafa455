"""The host half of the LM graph's one create path (csrc/gp_lm_groups.hpp: pair validation, slot assignment, record offsets) against a restatement in Python, without a
device and without loading anything into Python: tests/lm_groups_cases.cpp includes the header, is built with the host compiler and the address and undefined-behaviour
sanitizers, and run as a plain program on scripted cases."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gtsam_points_amd", "csrc")
BETWEEN, PRIOR = 0, 1

# (name, N, held, VGICP pairs, correspondence pairs, pose factors (kind, a, b))
CASES = [
    ("F=3 G=1, pose 0 held", 3, [1, 0, 0], [(0, 1), (1, 2), (0, 2)], [(0, 1)], []),
    ("F=1 G=3, all but pose 1 held", 3, [1, 0, 1], [(0, 1)], [(0, 1), (1, 2), (0, 2)], []),
    ("pose factors only, nothing held", 4, [0, 0, 0, 0], [], [], [(PRIOR, 0, -1), (BETWEEN, 0, 1), (BETWEEN, 1, 2), (BETWEEN, 2, 3)]),
    ("all three, a prior on a held pose", 4, [0, 1, 0, 0], [(3, 0)], [(2, 1), (1, 3)], [(PRIOR, 1, -1), (BETWEEN, 3, 2)]),
    ("VGICP only", 2, [1, 0], [(0, 1), (1, 0)], [], []),
    ("correspondence only", 2, [0, 1], [], [(1, 0)], []),
    ("every pose held", 3, [1, 1, 1], [(0, 1)], [(1, 2)], []),
    ("VGICP pair out of range", 3, [1, 0, 0], [(0, 1), (1, 3)], [(0, 1)], []),
    ("VGICP pair negative", 3, [1, 0, 0], [(-1, 1)], [], []),
    ("VGICP pair of a pose and itself", 3, [1, 0, 0], [(0, 1), (2, 2)], [], []),
    ("correspondence pair out of range", 3, [1, 0, 0], [(0, 1)], [(0, 1), (3, 0)], []),
    ("correspondence pair of a pose and itself", 3, [1, 0, 0], [], [(1, 1)], []),
    ("both groups bad: the VGICP one is named", 3, [1, 0, 0], [(0, 5)], [(7, 7)], []),
    ("bad pair AND every pose held: the pair is named", 2, [1, 1], [(0, 2)], [], []),
    ("no poses", 0, [], [], [], []),
]


def layout_ref(N, held, vg, corr, pose):
    """the layout as the header's comment states it"""
    slot, slots = [], 0
    for h in held:
        slot.append(-1 if h else slots)
        slots += 0 if h else 1
    factor_slots = []
    for name, pairs in (("pose_pairs", vg), ("corr_pairs", corr)):
        for t, s in pairs:
            if not (0 <= t < N and 0 <= s < N and t != s):
                return f"refused: {name} entries must be two different poses in [0, num_poses)"
            factor_slots += [slot[t], slot[s]]
    for kind, a, b in pose:
        factor_slots += [slot[a], slot[b]] if kind == BETWEEN else [-1, slot[a]]
    if slots == 0:
        return "refused: every pose is held"
    R = len(vg) + len(corr) + len(pose)
    return (f"slots={slots} offsets=0 {len(vg)} {len(vg) + len(corr)} records={R} slot=" + "".join(f"{v} " for v in slot) + "factor_slots=" + "".join(f"{v} " for v in factor_slots))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("lm_groups") / "lm_groups_cases")
    # the host compiler alone: no hipcc, no HIP include path -- the header must stand without them
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "lm_groups_cases.cpp"), "-o", exe])
    return exe


def test_layout_matches_its_restatement(program, tmp_path):
    lines, want = [], []
    for name, N, held, vg, corr, pose in CASES:
        flat = lambda rows: " ".join(str(v) for row in rows for v in row)
        lines.append(f"{N} {' '.join(map(str, held))} {len(vg)} {flat(vg)} {len(corr)} {flat(corr)} {len(pose)} {flat(pose)}")
        want.append(layout_ref(N, held, vg, corr, pose))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    run = subprocess.run([program, str(path)], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr  # (a sanitizer report goes to stderr and fails the run)
    got = run.stdout.splitlines()
    assert len(got) == len(want)
    for (name, *_), g, w in zip(CASES, got, want):
        assert g == w, name


def test_the_cases_decide_what_their_names_say():
    by = {name: layout_ref(N, held, vg, corr, pose) for name, N, held, vg, corr, pose in CASES}
    assert by["F=3 G=1, pose 0 held"] == "slots=2 offsets=0 3 4 records=4 slot=-1 0 1 factor_slots=-1 0 0 1 -1 1 -1 0 "
    assert by["all three, a prior on a held pose"] == "slots=3 offsets=0 1 3 records=5 slot=0 -1 1 2 factor_slots=2 0 1 -1 -1 2 -1 -1 2 1 "
    assert by["every pose held"] == by["no poses"] == "refused: every pose is held"
    assert by["both groups bad: the VGICP one is named"].startswith("refused: pose_pairs") and by["correspondence pair out of range"].startswith("refused: corr_pairs")
    assert by["bad pair AND every pose held: the pair is named"].startswith("refused: pose_pairs")
