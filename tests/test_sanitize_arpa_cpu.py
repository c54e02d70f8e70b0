"""CPU sanitizer pass (ASan + UBSan) over the host ARPA reader behind lasr_arpa_load (lightning_asr_amd/csrc/arpa_io.h, the SAME
source liblasr.so compiles): tests/sanitize/arpa_fuzz.cpp feeds it a good file, every truncation of it, thousands of byte and
line mutations, hostile counts and orders, overflowing numbers, KenLM's binary magic, empty and NUL files, and checks every
image it accepts for the consistency the search kernel relies on."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow,float-divide-by-zero", "-fno-sanitize-recover=all"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_arpa_reader_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "arpa_fuzz")
    b = subprocess.run(["g++"] + FLAGS + [os.path.join(ROOT, "tests", "sanitize", "arpa_fuzz.cpp"), "-o", exe], capture_output=True,
                       text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "arpa_fuzz ok" in r.stdout and "fuzz corpus:" in r.stderr


def test_library_wraps_the_sanitized_arpa_source():
    """ctc_beam.hip holds no ARPA parsing of its own: it includes arpa_io.h and wraps it; the header has no HIP"""
    src = open(os.path.join(ROOT, "lightning_asr_amd", "csrc", "ctc_beam.hip")).read()
    assert '#include "arpa_io.h"' in src and "host::arpa_load(" in src
    assert "strtod" not in src and "fopen" not in src
    hdr = open(os.path.join(ROOT, "lightning_asr_amd", "csrc", "arpa_io.h")).read()
    body = hdr.split("#pragma once", 1)[1]
    assert "hip_runtime" not in body and "__device__" not in body and "__global__" not in body
