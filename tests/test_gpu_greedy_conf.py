"""GPU tier of ops.greedy_confidence / ops.hyp_neg_logprob against the plain restatement of tests/helpers/greedy_conf_oracle.py.

Gates (include/lasr.h, lasr_greedy_confidence): tokens, n_tokens, tok_start, tok_end, tok_min, n_nonblank exact; utt_sum to
T * 2^-52 relative (same-sign terms: any summation order stays inside it); tok_mean and conf within 1 f32 ulp of the oracle's f64
value rounded to f32 (the f64 error is far below half an f32 ulp, so only a rounding boundary can differ).
Shapes are the smallest that can go wrong: the class counts either side of the row pass's switch of form and of the 16-byte
alignment cases, the frame counts either side of the collapse's tile."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import greedy_conf_oracle as O  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "pseudo_confidence.npz")
PAD = 50.0          # what padding frames past lens hold: any leak wins every max


def _geometry():
    from lightning_asr_amd import ops
    return ops.greedy_confidence_frame_tile(), ops.greedy_confidence_narrow_classes()


def _lens_for(B, T, tile):
    """T, 0, 1, and lengths that end the last run exactly on, just before and just after a tile border"""
    cand = [T, 0, 1, tile, tile - 1, tile + 1, 2 * tile, T - 1, T // 2, 3 * tile]
    return np.array([min(max(cand[i % len(cand)], 0), T) for i in range(B)], dtype=np.int32)


def _check(dev, logp, lens, blank):
    from lightning_asr_amd import ops
    B, T, C = logp.shape
    want = O.oracle(logp, lens, blank)
    lens_d = None if lens is None else torch.from_numpy(np.asarray(lens, dtype=np.int32)).to(dev)
    got = ops.greedy_confidence(torch.from_numpy(logp).to(dev), lens_d, blank)
    torch.cuda.synchronize()
    g = {k: getattr(got, k).cpu().numpy() for k in got._fields}
    for k in ("n_tokens", "n_nonblank", "tokens", "tok_start", "tok_end"):
        assert np.array_equal(g[k], want[k]), k
    assert np.array_equal(g["tok_min"], want["tok_min"]), "tok_min"
    err = O.rel_err(g["utt_sum"], want["utt_sum"])
    ulp_mean = int(O.ulp_distance(g["tok_mean"], want["tok_mean"]).max())
    ulp_conf = int(O.ulp_distance(g["conf"], want["conf"]).max())
    print("B=%d T=%d C=%d blank=%d: utt_sum rel err %.3g, tok_mean ulp %d, conf ulp %d" % (B, T, C, blank, err, ulp_mean, ulp_conf))
    assert err <= T * 2.0 ** -52
    assert ulp_mean <= 1 and ulp_conf <= 1
    return got, want


def _random_case(seed, B, T, C, tile, bias=None):
    blank = C - 1
    logp = O.make_logp(seed, B, T, C, blank, (np.log(C) + 1.0) if bias is None else bias)
    lens = _lens_for(B, T, tile)
    for b in range(B):
        logp[b, lens[b]:] = PAD
    return logp, lens, blank


def test_class_counts(dev):
    """C in {1, 2, 27, 28, 29, 4334, 4335} and the counts at and either side of the switch from rows that share a wave to a wave
    per row (the kernel's own constant); T = one tile + 1, so every utterance crosses a tile border"""
    tile, narrow = _geometry()
    counts = sorted({1, 2, 27, 28, 29, 4334, 4335, narrow - 1, narrow, narrow + 1,
                     narrow // 2, narrow // 2 + 1})           # (and either side of a power of two inside the shared-wave form)
    for C in counts:
        logp, lens, blank = _random_case(1000 + C, 3, tile + 1, C, tile)
        _check(dev, logp, lens, blank)


@pytest.mark.parametrize("B", [1, 3, 33])
def test_batch_and_frames(dev, B):
    """B in {1, 3, 33} x T in {1, 2, tile - 1, tile, tile + 1, 2001} at C = 28; lens hold 0, 1, T and the tile borders"""
    tile, narrow = _geometry()
    for T in (1, 2, tile - 1, tile, tile + 1, 2001):
        logp, lens, blank = _random_case(7 * B + T, B, T, 28, tile)
        _check(dev, logp, lens, blank)


def test_wide_rows_many_frames_and_no_lens(dev):
    """the wave-per-row form with more rows than one workgroup takes, several tiles, and lens = NULL"""
    tile, narrow = _geometry()
    logp, lens, blank = _random_case(5, 33, tile + 1, narrow + 1, tile)
    _check(dev, logp, lens, blank)
    logp, lens, blank = _random_case(6, 1, 2001, 4334, tile)
    _check(dev, logp, lens, blank)
    logp = O.make_logp(8, 3, 2 * tile + 5, 29, 28, 4.0)
    _check(dev, logp, None, 28)


def _constructed(tile):
    T, C = 2 * tile + 3, 5
    ninf = -np.inf
    rows, lens = [], []

    def row(winners, Tb=T, value=None):
        x = np.full((T, C), -9.0, np.float32)
        for t, c in enumerate(winners):
            if c is not None:
                x[t, c] = (-0.1 - 0.001 * t) if value is None else value(t)
        x[Tb:] = PAD
        rows.append(x)
        lens.append(Tb)
        return x

    row([4] * T)                                               # all "class 4" (all blank when blank = 4)
    row([1] * T)                                               # one label throughout: one run over every tile
    row([t % 2 for t in range(T)])                             # alternating labels
    row([0 if t % 2 == 0 else 4 for t in range(T)])            # label - blank - same label: a token each time
    w = [4] * T
    for t in range(tile - 3, tile + 5):                        # a run that crosses the tile border
        w[t] = 2
    for t in range(2 * tile - 4, 2 * tile):                    # a run that ends exactly on one
        w[t] = 1
    for t in range(2 * tile, 2 * tile + 2):                    # and one that starts exactly on one
        w[t] = 3
    row(w)
    x = row([None] * T)                                        # exact ties: two labels (1, 2 -> 1), a label and class 4 (3, 4 -> 3), class 0 and a label
    for t in range(T):
        pair = [(1, 2), (3, 4), (0, 3)][(t // 3) % 3]
        x[t, pair[0]] = x[t, pair[1]] = -0.25 - 0.001 * t
    x[T:] = PAD
    x = row([2] * T)                                           # frames of -inf only inside a label's run and at a tile border
    for t in (0, 5, 6, tile - 1, tile, T - 1):
        x[t] = ninf
    x = row([3] * T)                                           # -inf in some classes only
    x[:, 0] = ninf
    row([1 if (t // 7) % 2 else 4 for t in range(T)], Tb=tile + 44)      # lens < T, padding holds large values
    row([2] * T, Tb=tile)                                      # a run cut by lens exactly on the tile border
    x = row([4] * T)                                           # an utterance of -inf only
    x[:] = ninf
    return np.stack(rows), np.array(lens, np.int32)


@pytest.mark.parametrize("blank", [4, 0])
def test_constructed_rows(dev, blank):
    tile, _ = _geometry()
    logp, lens = _constructed(tile)
    got, want = _check(dev, logp, lens, blank)
    n = want["n_tokens"]
    T = logp.shape[1]
    if blank == 4:
        assert n[0] == 0 and n[1] == 1 and n[2] == T and n[3] == (T + 1) // 2 and n[4] == 3 and n[9] == 1
        assert want["tok_start"][4, :3].tolist() == [tile - 3, 2 * tile - 4, 2 * tile] and want["tok_end"][4, :3].tolist() == [tile + 5, 2 * tile, 2 * tile + 2]
        assert set(want["tokens"][5, :n[5]].tolist()) == {0, 1, 3}                 # every tie went to the smaller id
        assert want["tok_end"][9, 0] == tile and want["tok_end"][8, :n[8]].max() <= tile + 44
        assert np.isinf(want["conf"][10]).all() and np.isinf(want["utt_sum"][6]).all()
    else:
        assert n[1] == 1 and n[3] == T // 2 and n[10] == 0                       # rows of -inf only are class 0 = the blank here
        assert 0 not in set(want["tokens"][5, :n[5]].tolist())
        assert np.isinf(want["utt_sum"][6, 0]) and np.isfinite(want["utt_sum"][6, 1]) and want["conf"][10, 1] == O.confidence(0.0, 0)
    assert float(got.conf.cpu()[10, 0]) == float("inf")


def test_matches_greedy_decode_bit_for_bit(dev):
    from lightning_asr_amd import ops
    tile, narrow = _geometry()
    for B, T, C in ((5, 2 * tile + 9, 28), (2, tile + 3, narrow + 7)):
        logp, lens, blank = _random_case(31 + C, B, T, C, tile)
        x = torch.from_numpy(logp).to(dev)
        lens_d = torch.from_numpy(lens).to(dev)
        got = ops.greedy_confidence(x, lens_d, blank)
        tok, n = ops.greedy_decode(x.argmax(-1).to(torch.int32).contiguous(), lens_d, blank)
        assert torch.equal(got.tokens, tok) and torch.equal(got.n_tokens, n)


def test_reference_fixture(dev):
    """conf[0] is the reference's sum_logprob: within 1 ulp of its recorded f64 value rounded to f32"""
    from lightning_asr_amd import ops
    g = np.load(GOLD)
    for name in g["cases"]:
        seed, B, T, C = (int(v) for v in g[name + "_shape"])
        logp = O.make_logp(seed, B, T, C, C - 1, float(g[name + "_blank_bias"]))
        got = ops.greedy_confidence(torch.from_numpy(logp).to(dev), torch.from_numpy(g[name + "_lens"]).to(dev), C - 1)
        ulp = O.ulp_distance(got.conf[:, 0].cpu().numpy(), g[name + "_sum_logprob"])
        print(name, "ulp vs sum_logprob", ulp)
        assert ulp.max() <= 1


def test_posterior_measure(dev):
    from lightning_asr_amd import ops
    tile, narrow = _geometry()
    for B, T, C, bias in ((4, 60, 28, 3.0), (3, 40, narrow + 5, 5.0)):
        blank = C - 1
        logp = O.make_logp(77 + C, B, T, C, blank, bias)
        logp[0, :, :] = O.make_logp(3, 1, T, C, blank, 40.0)[0]               # an utterance whose hypothesis is empty
        lens = np.array([T, T - 7, T // 2, 3][:B], dtype=np.int32)
        x, lens_d = torch.from_numpy(logp).to(dev), torch.from_numpy(lens).to(dev)
        gc = ops.greedy_confidence(x, lens_d, blank)
        assert int(gc.n_tokens[0]) == 0 and int(gc.n_tokens.max()) > 0
        post = ops.hyp_neg_logprob(x, lens_d, gc.tokens, gc.n_tokens, blank)
        # by definition: ctc_loss of the hypothesis over (Tb + 1e-6)
        tg = gc.tokens.clamp(min=0).to(torch.int64).contiguous()
        nll, _ = ops.ctc_loss(x, tg, lens_d, gc.n_tokens, blank, want_grad=False)
        assert torch.equal(post, nll / (lens_d.float() + 1e-6))
        narrow_post = ops.hyp_neg_logprob(x, lens_d, gc.tokens, gc.n_tokens, blank, max_tokens=int(gc.n_tokens.max()))
        assert torch.allclose(post, narrow_post, rtol=1e-5, atol=0)
        # the empty hypothesis: -sum_t logp[t][blank] / (Tb + 1e-6)
        want0 = -float(logp[0, :lens[0], blank].astype(np.float64).sum()) / (lens[0] + 1e-6)
        assert abs(float(post[0]) - want0) <= 1e-5 * max(1.0, abs(want0))
        # the greedy path is ONE alignment of the hypothesis: posterior <= ref, with the project's CTC gate as the slack
        ref, nll_h, post_h = gc.conf[:, 0].cpu().numpy().astype(np.float64), nll.cpu().numpy().astype(np.float64), post.cpu().numpy()
        print("posterior", post_h, "ref", ref)
        assert (post_h <= ref + 1e-4 * np.maximum(1.0, nll_h) / (lens + 1e-6)).all()


def test_refused_calls_launch_nothing(dev):
    from lightning_asr_amd import _lib
    lib = _lib.load()
    B, T, C = 2, 5, 4
    x = torch.zeros(B, T, C, device=dev)
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device=dev)  # noqa: E731
    f32 = lambda *s: torch.full(s, -7.0, dtype=torch.float32, device=dev)  # noqa: E731
    outs = [i32(B, T), i32(B), i32(B, T), i32(B, T), f32(B, T), f32(B, T), torch.full((B, 2), -7.0, dtype=torch.float64, device=dev),
            i32(B), f32(B, 2)]
    nb = lib.lasr_greedy_confidence_workspace_bytes(B, T, C)
    assert nb == 8 * B * T
    ws = torch.zeros(nb, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(logp=x.data_ptr(), shape=(B, T, C), blank=C - 1, ptrs=None, wsp=ws.data_ptr(), wbytes=nb):
        ptrs = [o.data_ptr() for o in outs] if ptrs is None else ptrs
        return lib.lasr_greedy_confidence(logp, None, shape[0], shape[1], shape[2], blank, *ptrs, wsp, wbytes, stream)

    assert call(logp=None) == -1                                              # LASR_E_ARG / _SHAPE / _WORKSPACE = -1 / -2 / -3
    for k in range(len(outs)):
        ptrs = [o.data_ptr() for o in outs]
        ptrs[k] = None
        assert call(ptrs=ptrs) == -1, k
    assert call(wsp=None) == -1
    for blank in (-1, C):
        assert call(blank=blank) == -2
    for shape in ((0, T, C), (B, 0, C), (B, T, 0), (1 << 16, 1 << 15, C)):
        assert call(shape=shape) == -2, shape
        assert lib.lasr_greedy_confidence_workspace_bytes(*shape) == 0
    assert call(wbytes=nb - 1) == -3
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == -7).all()), "a refused call must not launch"
    assert call() == 0
    torch.cuda.synchronize()
    # all-equal rows: class 0 wins every tie, one run of it per utterance
    assert outs[1].tolist() == [1, 1] and outs[0][:, 0].tolist() == [0, 0] and outs[3][:, 0].tolist() == [T, T]
    assert not bool((outs[0] == -7).any())


def test_graph_capture_and_replay(dev):
    from lightning_asr_amd import ops
    tile, _ = _geometry()
    logp_a, lens, blank = _random_case(41, 3, tile + 9, 28, tile)
    logp_b = O.make_logp(42, 3, tile + 9, 28, blank, 2.0)
    x = torch.from_numpy(logp_a).to(dev)
    lens_d = torch.from_numpy(lens).to(dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.greedy_confidence(x, lens_d, blank)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = ops.greedy_confidence(x, lens_d, blank)
    for logp in (logp_a, logp_b):
        x.copy_(torch.from_numpy(logp))
        g.replay()
        torch.cuda.synchronize()
        want = O.oracle(logp, lens, blank)
        for k in ("tokens", "n_tokens", "tok_start", "tok_end", "tok_min", "n_nonblank"):
            assert np.array_equal(getattr(got, k).cpu().numpy(), want[k]), k
        assert O.ulp_distance(got.conf.cpu().numpy(), want["conf"]).max() <= 1
