"""CPU tier of the resumable CTC beam search (lasr_ctc_beam_stream_*): the version, the exported and declared symbols, the
size functions' ranges and the argument checks of feed and reset, all of which run before any launch and need no GPU."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("lasr_ctc_beam_stream_state_bytes", "lasr_ctc_beam_stream_workspace_bytes", "lasr_ctc_beam_stream_reset",
        "lasr_ctc_beam_stream_feed")
E_ARG, E_SHAPE, E_WORKSPACE = -1, -2, -3


def _lib():
    from lightning_asr_amd import _lib
    return _lib.load()


def test_version_and_symbols():
    from lightning_asr_amd import _lib
    lib = _lib.load()
    assert lib.lasr_version() >= 118
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lasr.h")).read(), flags=re.S)
    for s in SYMS:
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES
        assert re.search(r"\b%s\s*\(" % s, text), "%s is not declared in include/lasr.h" % s
    assert "lasr_beam_scorer" in text
    for k, name in enumerate(("PLAIN", "LM", "WLM", "BIAS", "LM_BIAS")):
        assert re.search(r"LASR_BEAM_%s = %d\b" % (name, k), text)
        assert getattr(_lib, "BEAM_" + name) == k


def test_state_and_workspace_ranges():
    lib = _lib()
    state, ws = lib.lasr_ctc_beam_stream_state_bytes, lib.lasr_ctc_beam_stream_workspace_bytes
    for kind in range(5):
        assert state(3, 100, 16, kind) > 0
        # header + an LDS image below 64 KB + the trie of 1 + T_cap * W nodes of 8 bytes, per stream
        per = state(1, 100, 16, kind)
        assert (1 + 100 * 16) * 8 < per < (1 + 100 * 16) * 8 + 64 + 65536 + 512
        assert state(3, 100, 16, kind) == 3 * per
    assert state(1, 100, 0, 0) == 0 and state(1, 100, 129, 0) == 0
    assert state(1, 100, 16, 5) == 0 and state(1, 100, 16, -1) == 0
    assert state(0, 100, 16, 0) == 0 and state(1, 0, 16, 0) == 0
    assert state(1, (1 << 31) // 128, 128, 0) == 0                     # 1 + T_cap * W = 2^31 + 1
    assert state(1, ((1 << 31) - 1) // 128, 128, 0) > 0                # 1 + T_cap * W = 2^31 - 127
    assert state(1, (1 << 31) - 1, 1, 0) == 0                          # 1 + T_cap * W = 2^31
    assert ws(3, 50, 28, 16, 40) > 0
    assert ws(3, 50, 28, 0, 40) == 0 and ws(3, 50, 28, 129, 40) == 0
    assert ws(3, 50, 8193, 16, 40) == 0 and ws(3, 50, 28, 16, 65) == 0 and ws(3, 0, 28, 16, 40) == 0
    # the kept lists of one chunk only: the one-shot workspace of the same shape also holds the trie
    assert ws(3, 50, 28, 16, 40) < lib.lasr_ctc_beam_workspace_bytes(3, 50, 28, 16, 40)
    assert ws(3, 50, 28, 128, 40) == ws(3, 50, 28, 16, 40)
    assert ws(3, 100, 28, 16, 40) > ws(3, 50, 28, 16, 40)


def _feed_caller(lib):
    from lightning_asr_amd import _lib
    fake = ctypes.c_void_p(4096)             # never dereferenced: every call below fails its checks before any launch
    base = dict(logp=fake, lens=None, B=2, T=10, C=28, blank=27, W=16, k=40, cp=1.0, n_best=1, kind=0, lm=None, alpha=1.0,
                beta=1.0, bias=None, am=None, bs=None, scorer=True, state=fake, sb=1 << 30, cap=100, tok=fake, n=fake, sc=fake,
                nf=fake, nd=fake, ws=fake, nb=1 << 20)

    def call(**kw):
        a = dict(base, **kw)
        s = _lib.BeamScorer(a["kind"], a["lm"], a["alpha"], a["beta"], a["bias"], a["am"], a["bs"])
        return lib.lasr_ctc_beam_stream_feed(a["logp"], a["lens"], a["B"], a["T"], a["C"], a["blank"], a["W"], a["k"], a["cp"],
                                             a["n_best"], ctypes.byref(s) if a["scorer"] else None, a["state"], a["sb"], a["cap"],
                                             a["tok"], a["n"], a["sc"], a["nf"], a["nd"], a["ws"], a["nb"], None)
    return call, fake


def test_feed_rejects_bad_arguments_without_a_gpu():
    lib = _lib()
    call, fake = _feed_caller(lib)
    for name in ("logp", "state", "tok", "n", "sc", "nf", "nd", "ws"):
        assert call(**{name: None}) == E_ARG, name
        assert b"null pointer" in lib.lasr_last_error() and b"lasr_ctc_beam_stream_feed" in lib.lasr_last_error()
    assert call(scorer=False) == E_ARG and b"null pointer" in lib.lasr_last_error()
    assert call(kind=5) == E_ARG and b"kind" in lib.lasr_last_error()
    assert call(kind=-1) == E_ARG
    # what each kind needs beside the common arguments
    assert call(kind=1) == E_ARG and b"null pointer" in lib.lasr_last_error()                  # no LM image
    assert call(kind=1, lm=fake) == E_ARG                                                        # no am_scores
    assert call(kind=2, lm=fake) == E_ARG
    assert call(kind=3, bias=fake, am=fake) == E_ARG                                             # no bias_scores
    assert call(kind=4, lm=fake, am=fake, bias=fake) == E_ARG
    assert call(kind=1, lm=fake, am=fake, alpha=float("nan")) == E_ARG and b"alpha" in lib.lasr_last_error()
    assert call(n_best=17) == E_ARG and b"n_best" in lib.lasr_last_error()
    assert call(n_best=0) == E_ARG
    assert call(cp=0.0) == E_ARG and b"cutoff_prob" in lib.lasr_last_error()
    assert call(cp=1.5) == E_ARG and call(cp=float("nan")) == E_ARG
    assert call(blank=28) == E_ARG and b"blank" in lib.lasr_last_error()
    assert call(blank=-1) == E_ARG
    assert call(W=129) == E_SHAPE and b"beam_width" in lib.lasr_last_error()
    assert call(k=65) == E_SHAPE
    assert call(C=8193, blank=0) == E_SHAPE
    assert call(T=0) == E_SHAPE
    assert call(cap=0) == E_SHAPE and b"T_cap" in lib.lasr_last_error()
    assert call(cap=1 << 28) == E_SHAPE                                                          # 1 + T_cap * 16 >= 2^31
    need = lib.lasr_ctc_beam_stream_state_bytes(2, 100, 16, 0)
    assert call(sb=need - 1) == E_WORKSPACE and b"state" in lib.lasr_last_error()
    assert call(nb=lib.lasr_ctc_beam_stream_workspace_bytes(2, 10, 28, 16, 40) - 1) == E_WORKSPACE
    assert b"workspace" in lib.lasr_last_error()


def test_reset_rejects_bad_arguments_without_a_gpu():
    lib = _lib()
    fake = ctypes.c_void_p(4096)
    need = lib.lasr_ctc_beam_stream_state_bytes(2, 100, 16, 0)
    reset = lib.lasr_ctc_beam_stream_reset
    assert reset(None, need, 2, 100, 16, 0, None, 0, None) == E_ARG and b"null pointer" in lib.lasr_last_error()
    assert reset(fake, need, 2, 100, 16, 0, None, 3, None) == E_ARG and b"n_rows" in lib.lasr_last_error()
    assert reset(fake, need, 2, 100, 16, 0, fake, -1, None) == E_ARG
    assert reset(fake, need, 2, 100, 129, 0, None, 0, None) == E_SHAPE and b"beam_width" in lib.lasr_last_error()
    assert reset(fake, need, 2, 100, 16, 7, None, 0, None) == E_SHAPE and b"kind" in lib.lasr_last_error()
    assert reset(fake, need, 2, 0, 16, 0, None, 0, None) == E_SHAPE
    assert reset(fake, need - 1, 2, 100, 16, 0, None, 0, None) == E_WORKSPACE and b"state" in lib.lasr_last_error()
    assert reset(fake, need, 2, 100, 16, 0, fake, 0, None) == 0          # no rows: nothing to launch


def test_stream_surface_without_a_gpu():
    from lightning_asr_amd import ops
    from lightning_asr_amd.beam_search import BeamSearchDecoderWithLM
    assert hasattr(BeamSearchDecoderWithLM, "open_stream")
    for kw in (dict(beam_width=129), dict(beam_width=4, n_best=5), dict(cutoff_prob=0.0), dict(blank=3), dict(t_cap=0),
               dict(n_streams=0), dict(cutoff_top_n=0)):
        a = dict(n_streams=1, n_classes=3, blank=2, beam_width=4, cutoff_top_n=40, cutoff_prob=1.0, n_best=1, t_cap=10)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.CtcBeamStream(**a)
    with pytest.raises(TypeError):
        ops.CtcBeamStream(1, 3, 2, lm="x.arpa")
    with pytest.raises(TypeError):
        ops.CtcBeamStream(1, 3, 2, bank=[[0, 1]])
    lens, add = ops._chunk_lens([5, 0, 9], 3, 7, "cpu")
    assert lens.tolist() == [5, 0, 9] and lens.dtype == torch.int32 and add == [5, 0, 7]
    assert ops._chunk_lens(None, 2, 7, "cpu") == (None, [7, 7])
    with pytest.raises(ValueError):
        ops._chunk_lens([1, 2], 3, 7, "cpu")
