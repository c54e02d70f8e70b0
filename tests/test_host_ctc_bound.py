"""CPU tier: the CTC label bound and the workspace sizes of the long-label (multi-wave) lattice, through the C ABI."""
import os
import re

import pytest

from lightning_asr_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _align(n, a=256):
    return (n + a - 1) // a * a


def _lattice_bytes(B, T, S):
    """alpha + beta rows and the same-label chains, as include/lasr.h describes them"""
    ss = 2 * S + 1
    if ss <= 64 * 16:
        ns = 4 if ss <= 256 else (8 if ss <= 512 else 16)
        pitch = 64 * ns
    else:
        pitch = 1024 * -(-ss // 1024)
    return _align(2 * B * T * pitch * 4) + _align(B * S * 2 * 4)


def test_header_bound_matches_host_constant():
    text = open(os.path.join(ROOT, "include", "lasr.h")).read()
    m = re.search(r"#define\s+LASR_CTC_MAX_LABELS\s+(\d+)", text)
    assert m and int(m.group(1)) == 2047 == ops.CTC_MAX_LABELS


@pytest.mark.parametrize("S", [1, 100, 127, 128, 255, 256, 511])
def test_one_wave_workspace_unchanged(S):
    lib = _lib.load()
    B, T = 32, 501
    ns = 4 if 2 * S + 1 <= 256 else (8 if 2 * S + 1 <= 512 else 16)
    assert lib.lasr_ctc_workspace_bytes(B, T, S) == _align(2 * B * T * 64 * ns * 4) + _align(B * S * 2 * 4)


def test_multi_wave_workspace_grows_with_waves():
    lib = _lib.load()
    B, T = 4, 300
    prev = lib.lasr_ctc_workspace_bytes(B, T, 511)
    for S, W in ((512, 2), (1023, 2), (1024, 3), (1535, 3), (1536, 4), (2047, 4)):
        n = lib.lasr_ctc_workspace_bytes(B, T, S)
        assert n == _lattice_bytes(B, T, S), S
        assert n >= 2 * B * T * 1024 * W * 4 and n > prev, S
        prev = n
    assert lib.lasr_ctc_workspace_bytes(B, T, 2048) == 0
    # B = 32 at the reference's 40 s dev clips (T' = 2001), two waves: about 1 GB of alpha + beta
    assert 1.0e9 < lib.lasr_ctc_workspace_bytes(32, 2001, 600) < 1.1e9


@pytest.mark.parametrize("C", [4334, 5207])
def test_lean_workspace_holds_lattice_and_emissions(C):
    lib = _lib.load()
    B, T = 4, 300
    for S in (100, 511, 512, 1023, 1024, 2047):
        n = lib.lasr_ctc_lean_workspace_bytes(B, T, C, S)
        assert n >= _lattice_bytes(B, T, S) + B * T * (S + 1) * 4, S
    assert lib.lasr_ctc_lean_workspace_bytes(B, T, C, 2048) == 0
