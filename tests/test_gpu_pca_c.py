"""tests/c/pca_caller.c: the principal axes from a C program that sees include/morna_hip.h alone.  -m gpu"""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_c_program_against_the_header_alone(tmp_path):
    """Compiled with gcc against the header alone, run as a process of its own."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, libdir = str(tmp_path / "pca_caller"), os.path.join(root, "morna_amd")
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Werror", "-std=c99", "-ffp-contract=off", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "c", "pca_caller.c"), "-o", exe, "-L", libdir, "-lmorna_hip",
                           "-Wl,-rpath," + libdir, "-lm"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pca caller ok" in r.stdout
