"""CPU sanitizer pass (ASan + UBSan) over the word-mode image builder behind lasr_arpa_load_words
(lightning_asr_amd/csrc/arpa_io.h, the SAME source liblasr.so compiles): tests/sanitize/arpa_words_fuzz.cpp feeds it a good
word-level file, every truncation of it, thousands of byte and line mutations, a word of thousands of code points, words of
invalid UTF-8, hostile vocabularies and space ids, and walks every image it accepts fully - the n-gram slots and the lexicon
from the root, with no probe leaving the table."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow,float-divide-by-zero", "-fno-sanitize-recover=all"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_arpa_word_builder_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "arpa_words_fuzz")
    b = subprocess.run(["g++"] + FLAGS + [os.path.join(ROOT, "tests", "sanitize", "arpa_words_fuzz.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "arpa_words_fuzz ok" in r.stdout and "fuzz corpus:" in r.stderr


def test_library_wraps_the_sanitized_word_builder():
    """ctc_beam.hip holds no image building of its own: lasr_arpa_load_words wraps arpa_io.h's arpa_load_words"""
    src = open(os.path.join(ROOT, "lightning_asr_amd", "csrc", "ctc_beam.hip")).read()
    assert "host::arpa_load_words(" in src and "ArpaLexHeader lh" not in src and "unordered_map" not in src
    hdr = open(os.path.join(ROOT, "lightning_asr_amd", "csrc", "arpa_io.h")).read()
    assert "arpa_parse_words" in hdr and "hip_runtime" not in hdr.split("#pragma once", 1)[1]
