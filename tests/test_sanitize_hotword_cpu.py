"""CPU sanitizer pass (ASan + UBSan) over the hotword bank behind lasr_hotword_build / lasr_hotword_score
(lightning_asr_amd/csrc/hotword_io.h, the SAME source liblasr.so compiles and whose walker its search kernels call):
tests/sanitize/hotword_fuzz.cpp builds a hand-made bank and 2 000 random ones, checks every image for the consistency the
kernels rely on, walks label sequences over a copy of each image, feeds the builder hostile arguments and the walker every
truncation and thousands of byte mutations of a good image."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow,float-divide-by-zero", "-fno-sanitize-recover=all"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_hotword_bank_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "hotword_fuzz")
    b = subprocess.run(["g++"] + FLAGS + [os.path.join(ROOT, "tests", "sanitize", "hotword_fuzz.cpp"), "-o", exe], capture_output=True,
                       text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "hotword_fuzz ok" in r.stdout and "fuzz corpus:" in r.stderr


def test_library_wraps_the_sanitized_hotword_source():
    """ctc_beam.hip holds no automaton of its own: it includes hotword_io.h, wraps its builder and calls its walker from the
    kernels; the header has no HIP header and no kernel"""
    src = open(os.path.join(ROOT, "lightning_asr_amd", "csrc", "ctc_beam.hip")).read()
    assert '#include "hotword_io.h"' in src and "host::hotword_build(" in src and "host::hotword_step(" in src
    hdr = open(os.path.join(ROOT, "lightning_asr_amd", "csrc", "hotword_io.h")).read()
    body = hdr.split("#pragma once", 1)[1]
    assert "hip_runtime" not in body and "__global__" not in body
    assert body.count("int hotword_step(") == 1
