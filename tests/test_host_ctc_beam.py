"""CPU tier of the CTC prefix beam search: the f64 oracle (tests/helpers/ctc_beam_oracle.py) against brute-force path
enumeration, and the C ABI's range / argument checks, which need no GPU."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import ctc_beam_oracle as O  # noqa: E402


def _cases(n=30, seed=0):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        T, C = int(rng.integers(1, 7)), int(rng.integers(2, 5))
        yield torch.log_softmax(torch.tensor(rng.normal(size=(T, C)) * 1.5), -1).numpy()


def test_oracle_unbounded_beam_is_exact():
    """beam = infinity, cutoff_top_n = C: the top entry is the most probable labelling, its score that labelling's exact
    log-likelihood, which is also -F.ctc_loss"""
    for x in _cases():
        T, C = x.shape
        exact = O.brute_force(x, C - 1)
        best = max(exact.items(), key=lambda kv: kv[1])
        hyps, _ = O.beam_search(x, T, C - 1, 10 ** 6, C, 1.0, 3)
        assert hyps[0][0] == best[0]
        assert hyps[0][1] == pytest.approx(best[1], abs=1e-12)
        for p, s in hyps:
            assert s == pytest.approx(exact[p], abs=1e-12)       # every prefix score is exact without pruning
        tgt = torch.tensor([list(best[0]) or [0]])
        nll = torch.nn.functional.ctc_loss(torch.tensor(x).unsqueeze(1), tgt, torch.tensor([T]), torch.tensor([len(best[0])]),
                                           blank=C - 1, reduction="none")
        assert -nll.item() == pytest.approx(best[1], abs=1e-9)


def test_oracle_scores_never_exceed_the_likelihood():
    for x in _cases(seed=1):
        T, C = x.shape
        exact = O.brute_force(x, C - 1)
        for W in (1, 2, 3):
            for k in (1, C):
                for cp in (1.0, 0.6):
                    hyps, _ = O.beam_search(x, T, C - 1, W, k, cp, W)
                    assert len({p for p, _ in hyps}) == len(hyps)
                    assert all(a[1] >= b[1] for a, b in zip(hyps, hyps[1:]))
                    for p, s in hyps:
                        assert s <= exact[p] + 1e-12


def test_oracle_pruning_order_and_cutoff_prob():
    row = np.log(np.array([0.1, 0.4, 0.1, 0.3, 0.1]))
    kept, _ = O.prune(row, 40, 1.0)
    assert kept == [1, 3, 0, 2, 4]                       # log-prob descending, ties by class id
    assert O.prune(row, 2, 1.0)[0] == [1, 3]
    assert O.prune(row, 40, 0.75)[0] == [1, 3, 0]        # 0.4 + 0.3 = 0.7 < 0.75 <= 0.8
    assert O.prune(row, 40, 0.7 - 1e-9)[0] == [1, 3]


def _lib():
    from lightning_asr_amd import _lib
    return _lib.load()


def test_beam_workspace_range():
    lib = _lib()
    for B, T, C, W, k in [(1, 1, 1, 1, 1), (32, 2001, 28, 128, 40), (4, 400, 4334, 16, 40), (2, 10, 8192, 64, 64),
                          (1, 50, 5207, 1, 1)]:
        assert lib.lasr_ctc_beam_workspace_bytes(B, T, C, W, k) > 0
    for B, T, C, W, k in [(2, 10, 28, 0, 40), (2, 10, 28, 129, 40), (2, 10, 28, 16, 65), (2, 10, 8193, 16, 40),
                          (2, 10, 28, 16, 0), (0, 10, 28, 16, 40), (2, 0, 28, 16, 40), (1, 1 << 24, 28, 128, 40)]:
        assert lib.lasr_ctc_beam_workspace_bytes(B, T, C, W, k) == 0, (B, T, C, W, k)
    # more frames, wider beams: never less room
    assert lib.lasr_ctc_beam_workspace_bytes(2, 20, 28, 16, 40) > lib.lasr_ctc_beam_workspace_bytes(2, 10, 28, 16, 40)
    assert lib.lasr_ctc_beam_workspace_bytes(2, 10, 28, 32, 40) > lib.lasr_ctc_beam_workspace_bytes(2, 10, 28, 16, 40)


def test_beam_decode_rejects_bad_arguments_without_a_gpu():
    lib = _lib()
    fake = ctypes.c_void_p(4096)             # never dereferenced: every call below fails its checks before any launch
    args = dict(logp=fake, lens=None, B=2, T=10, C=28, blank=27, W=16, k=40, cp=1.0, n_best=1, tok=fake, n=fake, sc=fake,
                ws=fake, nb=1 << 20)

    def call(**kw):
        a = dict(args, **kw)
        return lib.lasr_ctc_beam_decode(a["logp"], a["lens"], a["B"], a["T"], a["C"], a["blank"], a["W"], a["k"], a["cp"],
                                        a["n_best"], a["tok"], a["n"], a["sc"], a["ws"], a["nb"], None)
    for name in ("logp", "tok", "n", "sc", "ws"):
        assert call(**{name: None}) == -1, name
        assert b"null pointer" in lib.lasr_last_error()
    assert call(n_best=17) == -1 and b"n_best" in lib.lasr_last_error()
    assert call(n_best=0) == -1
    assert call(cp=0.0) == -1 and call(cp=1.5) == -1 and call(cp=float("nan")) == -1
    assert call(blank=28) == -1 and call(blank=-1) == -1
    assert call(W=129, n_best=1) == -2                           # LASR_E_SHAPE
    assert call(k=65) == -2
    assert call(C=8193, blank=0) == -2
    assert call(nb=16) == -3                                      # LASR_E_WORKSPACE


def test_beam_surface_without_a_gpu():
    from lightning_asr_amd import ops
    from lightning_asr_amd.beam_search import BeamSearchDecoderWithLM
    with pytest.raises(NotImplementedError):
        BeamSearchDecoderWithLM(["a", "b"], 8, 1.0, 1.0, "x.arpa", 4)
    dec = BeamSearchDecoderWithLM(["a", "b"], 8, 1.0, 1.0, None, 4, cutoff_prob=0.9, cutoff_top_n=10)
    assert dec.scorer is None and dec.beam_width == 8 and dec.cutoff_top_n == 10
    x = torch.zeros(1, 4, 3)
    with pytest.raises(ValueError):
        ops.ctc_beam_decode(x, None, 2, beam_width=129)
    with pytest.raises(ValueError):
        ops.ctc_beam_decode(x, None, 2, beam_width=4, n_best=5)
    with pytest.raises(ValueError):
        ops.ctc_beam_decode(torch.zeros(1, 4, 8193), None, 2)
    with pytest.raises(ValueError):
        ops.ctc_beam_decode(x, None, 2, cutoff_prob=0.0)
