"""The device-free arithmetic of the monolithic product (vasp_amd/csrc/fsi_product_host.hpp: the choice of forms from a refresh's
verdicts, the layout of the padded FP32 copy) in a stand-alone program (tests/product_host_check.cpp), built with the host compiler
and run on its own: it must report no failure.  The same program under -fsanitize=address,undefined is a run by hand on a
machine without a GPU (the command is in the program's header and in NOTEBOOK section 21), not part of the suite."""
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_forms_and_padded_layout(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "product_host_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'vasp_amd' / 'csrc'}",
                    str(ROOT / "tests" / "product_host_check.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("0 failures"), (run.stdout, run.stderr)
