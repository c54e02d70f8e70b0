"""CPU sanitizer pass (ASan + UBSan) over the host side of the voice-activity segmenter (lightning_asr_amd/csrc/segment.h, the SAME
source liblasr.so compiles): tests/sanitize/segment_fuzz.cpp - a stand-alone program with its own main - checks level() against a
bit-by-bit reference over the powers of two, their neighbours and the loudest frame, the known answers and round trips of the
parameter conversion, and feeds it hostile dB, seconds, permille and lengths.  Never run on the GPU, never loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow,float-divide-by-zero", "-fno-sanitize-recover=all"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_segment_host_side_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "segment_fuzz")
    b = subprocess.run(["g++"] + FLAGS + [os.path.join(ROOT, "tests", "sanitize", "segment_fuzz.cpp"), "-o", exe], capture_output=True,
                       text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "segment_fuzz ok" in r.stdout and "fuzz corpus:" in r.stderr


def test_library_wraps_the_sanitized_segment_source():
    """segment.hip converts and checks no parameter of its own and has no level function of its own: it includes segment.h and
    calls it, from the host wrappers and from the kernels; the header has no HIP"""
    src = open(os.path.join(ROOT, "lightning_asr_amd", "csrc", "segment.hip")).read()
    assert '#include "segment.h"' in src and "segment::from(" in src and "segment::check(" in src and "segment::level(" in src
    assert "log10" not in src and "pow(" not in src and "clz" not in src
    hdr = open(os.path.join(ROOT, "lightning_asr_amd", "csrc", "segment.h")).read()
    body = hdr.split("#pragma once", 1)[1]
    assert "hip_runtime" not in body and "__device__" not in body and "__global__" not in body
