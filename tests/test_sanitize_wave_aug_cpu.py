"""CPU sanitizer pass (ASan + UBSan) over the RIR bank builder behind lasr_rir_bank_bytes / _bank_write
(lightning_asr_amd/csrc/wave_aug.h, the SAME source liblasr.so compiles): tests/sanitize/wave_aug_fuzz.cpp - a stand-alone program
with its own main - checks known RIRs, feeds the builder hostile RIR sets, writes a thousand random banks from exactly sized source
blocks into exactly sized heap blocks and checks every header field the kernel relies on.  Never run on the GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow,float-divide-by-zero", "-fno-sanitize-recover=all"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_rir_bank_builder_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "wave_aug_fuzz")
    b = subprocess.run(["g++"] + FLAGS + [os.path.join(ROOT, "tests", "sanitize", "wave_aug_fuzz.cpp"), "-o", exe], capture_output=True,
                       text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "wave_aug_fuzz ok" in r.stdout and "fuzz corpus:" in r.stderr


def test_library_wraps_the_sanitized_wave_aug_source():
    """wave_aug.hip builds no bank of its own: it includes wave_aug.h and wraps it; the header has no HIP"""
    src = open(os.path.join(ROOT, "lightning_asr_amd", "csrc", "wave_aug.hip")).read()
    assert '#include "wave_aug.h"' in src and "wave_aug::bank_write(" in src and "wave_aug::bank_bytes(" in src and "wave_aug::entry_ok(" in src
    hdr = open(os.path.join(ROOT, "lightning_asr_amd", "csrc", "wave_aug.h")).read()
    body = hdr.split("#pragma once", 1)[1]
    assert "hip_runtime" not in body and "__device__" not in body and "__global__" not in body
