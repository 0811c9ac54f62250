"""csrc/core_side.h: which side a metric core is compiled for is the compiler's to say.  Every *_core.h and ordered_sum.h compiles as
the FIRST and only include of a translation unit, as plain C++ (the host drivers' side) and as HIP for gfx950 (the device pass of a
.hip), and nothing in csrc/ or tests/ spells a side by hand any more."""
import glob
import os
import re
import subprocess

import pytest

import host_program

CSRC = os.path.join(host_program.ROOT, "climate2weather_amd", "csrc")
HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*_core.h"))) + ["ordered_sum.h"]


def test_the_twelve_cores_and_the_ordered_sum_are_all_here():
    assert len(HEADERS) == 13, HEADERS


@pytest.mark.parametrize("header", HEADERS)
def test_a_core_compiles_as_the_first_include_on_either_side(tmp_path, header):
    unit = tmp_path / "unit.cpp"
    unit.write_text(f'#include "{header}"\n')
    subprocess.run(host_program.cxx() + ["-std=c++17", "-fsyntax-only", "-I" + CSRC, str(unit)], check=True, timeout=300)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "--cuda-device-only", "-fsyntax-only", "-std=c++17", "-I" + CSRC, str(unit)],
                   check=True, timeout=300)


def test_no_translation_unit_defines_a_side_by_hand():
    private = re.compile(r"\b(CRPS|ESC|EV|KDE|QMAP|QNT|SPEC|SP|SSIM|SWD|TINCR|WIND|ORDERED_SUM)_(HD|BOTH|HOST)\b")
    defines = re.compile(r"#define C2W_(HD|BOTH|CORE_HOST)")
    found = []
    for folder in (CSRC, os.path.join(host_program.ROOT, "tests")):
        for path in sorted(glob.glob(os.path.join(folder, "*"))):
            if not os.path.isfile(path) or not path.endswith((".h", ".hip", ".cpp", ".py")):
                continue
            with open(path, errors="replace") as f:
                text = f.read()
            if private.search(text) or (defines.search(text) and os.path.basename(path) != "core_side.h"):
                found.append(os.path.relpath(path, host_program.ROOT))
    assert not found, found
