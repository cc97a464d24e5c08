"""The leaf table of k_trace's flat scan on the CPU (libyafaray_amd/csrc/bvh.cc buildFlatTable, checked by
tests/flat_table_check.cc on the project's own builder): every triangle slot exactly once, every box equal to its
parent's stored child box bit for bit, the leaf count and word ranges as the tree says, and the eligibility
function's limits (65 triangles, a leaf count above the automatic limit).  Scenes: the Cornell box, cornell-fan
(slots in both mask words), cornell-fan with leaves of up to 8, dust of 33 / 64 triangles (bit 32, bit 63), dust of
64 with leaves of up to 8 (one leaf across slots 31 / 32: the table's middle range) and dust of 65 (no table)."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import raylib
from libyafaray_amd import scenes
from test_trace_deferred import cornell_fan

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "libyafaray_amd", "csrc")

CASES = {
    "cornell": (lambda: scenes.cornell(32, 32, spp=1), 1),
    "cornell-fan": (cornell_fan, 1),
    "cornell-fan-leaf8": (cornell_fan, 8),
    "dust-33": (lambda: raylib.dust(n=33), 1),
    "dust-64": (lambda: raylib.dust(n=64), 1),
    "dust-64-leaf8": (lambda: raylib.dust(n=64), 8),
    "dust-65": (lambda: raylib.dust(n=65), 1),
}


@pytest.fixture(scope="module")
def checker():
    exe = os.path.join(tempfile.mkdtemp(prefix="yaf_flat_"), "flat_table_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "flat_table_check.cc"),
                    os.path.join(CSRC, "bvh.cc"), "-lpthread"], check=True)
    return exe


@pytest.mark.parametrize("case", list(CASES))
def test_flat_table_of_the_builders_tree(checker, case, tmp_path):
    make, leaf = CASES[case]
    spec = make()
    verts = np.ascontiguousarray(spec.verts, np.float32)
    tris = np.ascontiguousarray(spec.tris, np.int32)
    mesh = tmp_path / "mesh.bin"
    with open(mesh, "wb") as f:
        f.write(np.array([len(verts), len(tris)], np.int32).tobytes())
        f.write(verts.tobytes())
        f.write(tris.tobytes())
    r = subprocess.run([checker, str(mesh), str(leaf)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    if case == "dust-65":
        assert "no table" in r.stdout
    if case == "cornell":
        assert "L = 21 " in r.stdout, r.stdout
    if case == "dust-64-leaf8":
        assert "/ 1 /" in r.stdout and "largest leaf 8" in r.stdout, r.stdout   # the leaf across both mask words
