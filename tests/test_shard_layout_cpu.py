"""The host arithmetic of the multi-GPU batch (csrc/gp_shard_layout.hpp: the layout of an assignment of factors to shards, the all-gather's send offsets, the balanced
contiguous plan) against a restatement in Python, without a device and without loading anything into Python: tests/shard_layout_cases.cpp includes the header, is
built with the host compiler and the address and undefined-behaviour sanitizers, and run as a plain program on scripted cases."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gtsam_points_amd", "csrc")

# (name, shard_of, num_shards)
LAYOUTS = [
    ("F=0, one shard", [], 1),
    ("F=0, three shards", [], 3),
    ("F=1 N=1", [0], 1),
    ("F=6 N=2, equal halves", [0, 0, 0, 1, 1, 1], 2),
    ("F=6 N=4, not divisible", [0, 0, 1, 1, 2, 3], 4),
    ("F=10 round-robin over 3", [i % 3 for i in range(10)], 3),
    ("equal ranges in the wrong rank order", [1, 1, 1, 0, 0, 0], 2),
    ("an empty shard between two with factors", [0, 0, 0, 2, 2, 2], 3),
    ("a contiguous shard beside a non-contiguous one", [0, 0, 0, 1, 2, 1, 2, 1, 2, 1], 3),
    ("shard index -1", [0, -1, 1], 2),
    ("shard index equal to N", [0, 1, 2], 2),
]
WIDTHS = (1, 122)

WEIGHTS = [[3, 1, 4, 1, 5, 9, 2], [1] * 7, [0] * 7, [100, 1, 1, 1, 1, 1, 1], [1, 2, 3, 4, 5, 6, 7], [7, 6, 5, 4, 3, 2, 1], [0, 5, 0, 5, 0, 5, 0]]
# (name, weights, k)
BOUNDARIES = [
    ("n=0", [], 3),
    ("k=1", [4, 2, 9], 1),
    ("n<k", [5, 6], 4),
    ("all weights zero", [0, 0, 0, 0, 0], 3),
    ("one weight larger than the rest together", [1, 2, 50, 3, 4], 3),
    ("equal weights", [5] * 6, 3),
] + [(f"sweep {w[:n]} k={k}", w[:n], k) for w in WEIGHTS for n in range(8) for k in range(1, 5)]


def layout_ref(shard_of, N, width):
    """the layout as the header's comments state it"""
    F = len(shard_of)
    if any(not 0 <= s < N for s in shard_of):
        return "refused: shard index out of range"
    lists = [[i for i in range(F) if shard_of[i] == k] for k in range(N)]
    contiguous = [ix == list(range(ix[0], ix[0] + len(ix))) if ix else True for ix in lists]
    rows = F // N if F > 0 and F % N == 0 and all(c and ix == list(range(k * (F // N), (k + 1) * (F // N))) for k, (c, ix) in enumerate(zip(contiguous, lists))) else 0
    out = f"rows={rows}"
    for ix, c in zip(lists, contiguous):
        first = ix[0] if ix else 0
        out += f" | first={first} contiguous={int(c)} offset={first * width} index=" + "".join(f"{v} " for v in ix)
    return out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("shard_layout") / "shard_layout_cases")
    # the host compiler alone: no hipcc, no HIP include path -- the header must stand without them
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "shard_layout_cases.cpp"), "-o", exe])
    return exe


def run_cases(program, tmp_path, lines):
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    run = subprocess.run([program, str(path)], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr  # (a sanitizer report goes to stderr and fails the run)
    got = run.stdout.splitlines()
    assert len(got) == len(lines)
    return got


def test_layout_matches_its_restatement(program, tmp_path):
    cases = [(name, so, N, width) for name, so, N in LAYOUTS for width in WIDTHS]
    got = run_cases(program, tmp_path, [f"L {len(so)} {N} {width} {' '.join(map(str, so))}" for _, so, N, width in cases])
    for (name, so, N, width), g in zip(cases, got):
        assert g == layout_ref(so, N, width), (name, width)


def test_the_layout_cases_decide_what_their_names_say():
    by = {(name, width): layout_ref(so, N, width) for name, so, N in LAYOUTS for width in WIDTHS}
    assert by["F=0, three shards", 122] == "rows=0" + " | first=0 contiguous=1 offset=0 index=" * 3
    assert by["F=1 N=1", 1] == "rows=1 | first=0 contiguous=1 offset=0 index=0 "
    assert by["F=6 N=2, equal halves", 122] == "rows=3 | first=0 contiguous=1 offset=0 index=0 1 2  | first=3 contiguous=1 offset=366 index=3 4 5 "
    assert by["F=6 N=2, equal halves", 1].count("offset=3 ") == 1
    for name in ["F=6 N=4, not divisible", "F=10 round-robin over 3", "equal ranges in the wrong rank order", "an empty shard between two with factors",
                 "a contiguous shard beside a non-contiguous one"]:
        assert by[name, 122].startswith("rows=0 |"), name
    assert by["F=10 round-robin over 3", 1].count("contiguous=0") == 3
    assert by["equal ranges in the wrong rank order", 122].startswith("rows=0 | first=3 contiguous=1 offset=366 ")
    assert " | first=0 contiguous=1 offset=0 index= | " in by["an empty shard between two with factors", 122]
    assert [g.split()[1] for g in by["a contiguous shard beside a non-contiguous one", 1].split(" | ")[1:]] == ["contiguous=1", "contiguous=0", "contiguous=0"]
    assert by["shard index -1", 1] == by["shard index equal to N", 122] == "refused: shard index out of range"  # the wording of gp_vgicp_multi_batch_create's refusal


def test_boundaries_are_optimal_and_leave_no_shard_empty(program, tmp_path):
    """what tests/test_distributed_cpu.py::test_shard_plan_is_optimal_and_leaves_no_shard_empty holds through the library, here under the sanitizers: a complete
    contiguous partition whose largest range sum is the brute-force optimum, with max(0, k - n) empty ranges"""
    got = run_cases(program, tmp_path, [f"B {len(w)} {k} {' '.join(map(str, w))}" for _, w, k in BOUNDARIES])
    by = {}
    for (name, w, k), g in zip(BOUNDARIES, got):
        assert g.startswith("begin=")
        b = [int(v) for v in g[len("begin="):].split()]
        by[name] = b
        n = len(w)
        assert len(b) == k + 1 and b[0] == 0 and b[-1] == n and all(lo <= hi for lo, hi in zip(b, b[1:])), (name, b)
        worst = max(sum(w[lo:hi]) for lo, hi in zip(b, b[1:]))
        best = min(max(sum(w[lo:hi]) for lo, hi in zip((0,) + cut, cut + (n,))) for cut in itertools.combinations_with_replacement(range(n + 1), k - 1))
        assert worst == best, (name, b)
        assert sum(1 for lo, hi in zip(b, b[1:]) if lo == hi) == max(0, k - n), (name, b)
    assert by["n=0"] == [0, 0, 0, 0] and by["k=1"] == [0, 3] and by["n<k"] == [0, 1, 2, 2, 2] and by["equal weights"] == [0, 2, 4, 6]
    assert by["one weight larger than the rest together"] == [0, 2, 3, 5]  # the heavy factor alone: the only partition whose largest sum is 50
