"""CPU check of the model lowering (pcp_amd/csrc/pcp_lower.hip): tests/lower_check.cpp compares every table the lowering builds with values
written out by hand from the format comments.  The checker is a program of its own, built with plain g++ under AddressSanitizer and UBSan
and run as a child process; nothing is loaded into this interpreter and no GPU is involved."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["records and constants", "sum views", "binary model payloads", "word descriptors", "Rec8", "all-different detection", "formula trees",
         "lower_big", "validators"]


def test_lowering_matches_the_table_formats():
    exe = os.path.join(ROOT, "tests", "lower_check")
    subprocess.run(["g++", "-x", "c++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                    "-o", exe, "tests/lower_check.cpp", "pcp_amd/csrc/pcp_lower.hip"], cwd=ROOT, check=True)
    r = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr  # (a sanitizer report)
    assert r.stdout.splitlines() == [f"ok {c}" for c in CASES] + ["all ok"]
