"""The shared spatial-keying code on the host, without a device and without loading anything into Python: tests/key_table_cases.cpp includes csrc/gp_key_table.hpp
(key_find / key_claim: the loops the kernels run, bounded at mask + 1 probes) and csrc/gp_cells.hpp (cell_of, CellBox) alone, is built with the host compiler
under AddressSanitizer and UBSan, and runs as a plain program.  Its cases: a 1-slot table, eight keys of one home slot running across the end of the table, a
claim of a stored key, a full table (no room / not found after exactly mask + 1 probes), a damaged table holding a key twice; cell_of at +-1e9, one ulp inside,
NaN, +-inf, -0.0, -1e-300 and 0.5 against std::floor in f64; the neutral CellBox and its folds.

The placement case ties the table to tests/fpfh_ref.py: 40 keys claimed one after another with hash_key land in the slots table_placement gives the same keys
(tests/golden/key_table_placement.json holds cells, keys, home slots and slots; the restatement is run again here, so the fixture cannot drift from it)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import fpfh_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gtsam_points_amd", "csrc")
FIXTURE = os.path.join(ROOT, "tests", "golden", "key_table_placement.json")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("key_table") / "key_table_cases")
    # the host compiler alone: no hipcc, no HIP include path -- the two headers must stand without them
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "key_table_cases.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def placement():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_is_the_restatements_table(placement):
    cells = np.array(placement["cells"], np.int64)
    assert cells.shape == (40, 3)
    points = ((cells + 0.5) * placement["radius"]).astype(np.float32)
    t = fpfh_ref.table_placement(points, placement["radius"])
    assert t["mask"] == placement["mask"] and (t["cells"] == cells).all()
    assert t["keys"].tolist() == placement["keys"] and t["home"].tolist() == placement["home"] and t["slot"].tolist() == placement["slot"]
    # what the set is there for: a crowded home slot, and a run across the end of the table
    assert np.bincount(t["home"]).max() >= 8 and t["wrapped"].sum() >= 3 and t["probes"].max() >= 8


def test_cases_and_placement(program, placement, tmp_path):
    path = tmp_path / "placement.txt"
    path.write_text(f"{placement['mask']}\n" + "".join(f"{k} {s}\n" for k, s in zip(placement["keys"], placement["slot"])))
    run = subprocess.run([program, str(path)], capture_output=True, text=True)
    lines = run.stdout.splitlines()
    failed = [ln for ln in lines if ln.startswith("FAIL")]
    assert run.returncode == 0 and not run.stderr and not failed, "\n".join(failed) + run.stderr  # (a sanitizer report goes to stderr and fails the run)
    placed = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith("placed")]
    assert placed == list(zip(placement["keys"], placement["slot"]))
    ok = [ln[3:] for ln in lines if ln.startswith("ok ")]
    # every case the program is there for has run (a case cannot pass by not being reached)
    for needle in ["one slot: claim", "shared home slot: the keys fill", "claiming a stored key", "full table: claim finds no room after exactly mask + 1 probes",
                   "full table: find gives -1 after exactly mask + 1 probes", "damaged table: find takes the first copy", "cell_of: u = 1e9 has no cell",
                   "cell_of: u = -1e9 has no cell", "cell_of: nextafter(1e9, 0) has a cell", "cell_of: NaN has no cell", "cell_of: +inf has no cell",
                   "cell_of: -inf has no cell", "cell_of: -0.0 is in cell 0", "cell_of: -1e-300 is in cell -1", "cell_of: 0.5 is in cell 0",
                   "CellBox: the neutral box is empty", "CellBox: folding neutral boxes stays empty", "CellBox: add then fold gives min / max per axis",
                   "placement: the keys land where the restatement puts them"]:
        assert any(name.startswith(needle) for name in ok), needle
