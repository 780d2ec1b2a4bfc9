"""The HOST staging layout (csrc/tpc_mpc_stage.h) under the address sanitizer: tests/stage_layout_main.cpp, a stand-alone
host program with its own main and no HIP call, lays out the compact entries' tables for every subset of their optional
arrays and writes every row the staging copies would touch into a heap buffer of exactly the computed size."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_stage_layout_under_the_address_sanitizer(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = tmp_path / "stage_layout"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(HERE, "stage_layout_main.cpp"), "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("stage layout ok")
