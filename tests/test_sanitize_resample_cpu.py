"""CPU sanitizer pass (ASan + UBSan) over the resampler's bank builder behind lasr_resample_bank_bytes / _bank_write / _out_len
(lightning_asr_amd/csrc/resample.h, the SAME source liblasr.so compiles): tests/sanitize/resample_fuzz.cpp - a stand-alone program
with its own main - checks known geometries and per-phase tap sums, feeds the builder hostile rates and limits, writes a thousand
random banks into exactly sized heap blocks and checks every header for what the kernel relies on.  Never run on the GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow,float-divide-by-zero", "-fno-sanitize-recover=all"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_resample_bank_builder_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "resample_fuzz")
    b = subprocess.run(["g++"] + FLAGS + [os.path.join(ROOT, "tests", "sanitize", "resample_fuzz.cpp"), "-o", exe], capture_output=True,
                       text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "resample_fuzz ok" in r.stdout and "fuzz corpus:" in r.stderr


def test_library_wraps_the_sanitized_resample_source():
    """resample.hip builds no filter of its own: it includes resample.h and wraps it; the header has no HIP"""
    src = open(os.path.join(ROOT, "lightning_asr_amd", "csrc", "resample.hip")).read()
    assert '#include "resample.h"' in src and "resample::bank_write(" in src and "resample::out_len(" in src
    assert "sin(" not in src and "cos(" not in src
    hdr = open(os.path.join(ROOT, "lightning_asr_amd", "csrc", "resample.h")).read()
    body = hdr.split("#pragma once", 1)[1]
    assert "hip_runtime" not in body and "__device__" not in body and "__global__" not in body
