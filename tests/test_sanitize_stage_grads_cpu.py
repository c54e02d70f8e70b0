"""CPU sanitizer pass (ASan + UBSan) over the collector of a backward stage's deferred gradients (lightning_asr_amd/csrc/stage_grads.h,
the SAME source model.hip compiles): tests/sanitize/stage_grads_check.cpp - a stand-alone program with its own main - drives it with a
recording launcher through the capacity branches the shipped models never reach, and replays the plain and the context model's
stages against the launches the step makes for them.  Never run on the GPU, never loaded into Python."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lightning_asr_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow,float-divide-by-zero", "-fno-sanitize-recover=all"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_stage_collector_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "stage_grads_check")
    b = subprocess.run(["g++"] + FLAGS + ["-Wall", os.path.join(ROOT, "tests", "sanitize", "stage_grads_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "stage_grads_check ok" in r.stdout


def test_model_step_keeps_its_deferred_gradients_in_the_collector():
    """model.hip includes the sanitized header and holds no list or capacity of its own; the header has no HIP; the capacities are
    defined once and used by the kernels' argument structs, the launchers' checks and the collector's launcher"""
    src = open(os.path.join(CSRC, "model.hip")).read()
    assert '#include "stage_grads.h"' in src and "StageGrads<StageLaunch>" in src
    assert "kMaxProblems = kMaxMultiProblems, kMaxSegments = kMaxReduceSegments" in src
    assert "std::vector<lasr_reduce_desc>" not in src and "std::vector<lasr_gemm_problem>" not in src and "splits[32]" not in src
    body = src.split("static int backward_from_glogits(", 1)[1].split("\nextern \"C\"", 1)[0]
    assert not re.search(r"push_back|\.erase\(|\.size\(\) [<>+]|> 60|> 32|> 64", body)
    hdr = open(os.path.join(CSRC, "stage_grads.h")).read().split("#pragma once", 1)[1]
    assert re.findall(r'#include ([<"][^>"]+[>"])', hdr) == ['"../../include/lasr.h"', "<vector>"]
    assert "hip_runtime" not in hdr and "__device__" not in hdr and "__global__" not in hdr
    gemm_h, fused_h = open(os.path.join(CSRC, "gemm.h")).read(), open(os.path.join(CSRC, "fused.h")).read()
    assert len(re.findall(r"constexpr int kMaxMultiProblems = 32;", gemm_h)) == 1 and "constexpr int kMaxMultiRiders = 24;" in gemm_h
    assert "constexpr int kMaxReduceSegments = 64;" in fused_h
    gemm_bf16, norm = open(os.path.join(CSRC, "gemm_bf16.hip")).read(), open(os.path.join(CSRC, "norm.hip")).read()
    assert "Bf16Args p[kMaxMultiProblems]" in gemm_bf16 and "rd[kMaxMultiRiders]" in gemm_bf16 and "n > kMaxMultiProblems" in gemm_bf16
    assert "lasr_reduce_desc d[kMaxReduceSegments]" in norm and "n_descs <= lasr::kMaxReduceSegments" in norm
