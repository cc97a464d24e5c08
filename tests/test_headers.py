"""The shared device headers of libyafaray_amd/csrc stand alone: each compiles for gfx950 as the first and only
include of an otherwise empty HIP file, so a header that leans on what its includer happened to include before it
fails here and not in some later unit.  Syntax only (no code generation): a few seconds on a CPU."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libyafaray_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HEADERS = ["camera.h", "filmmath.h", "launch.h", "trace.h"]


def test_shared_headers_compile_alone(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail(f"{HIPCC} not found: the device headers cannot be checked")

    def check(h):
        src = tmp_path / (h.replace(".", "_") + ".hip")
        src.write_text(f'#include "{h}"\n')
        return h, subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function",
                                  "-Wno-unused-variable", "-fsyntax-only", f"-I{CSRC}", str(src)], capture_output=True, text=True)

    with ThreadPoolExecutor(max_workers=4) as pool:
        results = list(pool.map(check, HEADERS))
    bad = [f"{h}:\n{r.stderr[-2000:]}" for h, r in results if r.returncode != 0]
    assert not bad, "\n".join(bad)


def test_no_device_variable_in_a_header():
    """Without relocatable device code a __device__ variable defined in a header is one variable per unit that
    includes it, and a host reader sees only its own unit's copy: every one is defined in a .hip file."""
    import re
    text = {n: open(os.path.join(CSRC, n)).read() for n in sorted(os.listdir(CSRC)) if n.endswith((".h", ".hip"))}
    pat = re.compile(r"^\s*(?:static\s+)?__device__\s+(?!__forceinline__|inline|__host__)[\w:<> ]+?\b\w+\s*(?:\[[^\]]*\])?\s*(?:=[^;(]*)?;", re.M)
    assert len(pat.findall(text["kernels.hip"])) >= 2   # the pattern sees kernels.hip's own (stage guard, phase cycles)
    found = [f"{h}: {m.group(0).strip()}" for h in text if h.endswith(".h") for m in pat.finditer(text[h])]
    assert not found, found
