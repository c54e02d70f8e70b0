"""The resumable CTC beam search (ops.CtcBeamStream, lasr_ctc_beam_stream_*) against the library's own one-shot decode of the
concatenated frames, which the other beam tests pin to the Python oracles.  The contract is bit-exact, so every comparison is
torch.equal on tokens, n_tokens and the f32 score tensors: chunk sizes of every kind, each scorer, the prefix property, a reset
in mid-stream, the capacity clamp, graph capture, and GreedyStream against ops.greedy_decode."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import arpa_synth as S  # noqa: E402
import wlm_synth as WS  # noqa: E402

pytestmark = pytest.mark.gpu

EN = ["'"] + [chr(ord("a") + i) for i in range(26)]               # data/labels.txt: C = 28 with the blank
WVOCAB = [" ", "a", "b", "c", "d"]                                 # the word LM's labels: C = 6 with the blank
WORDS = ["a", "ab", "abc", "aa", "abba", "b", "bad", "cab", "dad", "add", "cad", "dab"]
B, T, C = 3, 61, 28
LENS = [61, 37, 0]
FRAME_CHUNKS = {"frame_by_frame": [1] * 61, "uneven": [5, 1, 17, 38], "whole": [61]}
# per feed, the frames each stream takes: stream 1 idles in feeds 0 and 3, stream 2 always, stream 0 in feed 2
RAGGED = [[9, 0, 0], [20, 30, 0], [0, 7, 0], [31, 0, 0], [1, 0, 0]]


def peaky(Bn, Tn, Cn, seed, hot=6.0, sd=2.0, p_blank=0.5):
    """random log-softmax rows with one favoured class per frame, so that hypotheses carry labels"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(Bn, Tn, Cn, generator=g) * sd
    hotc = torch.randint(0, Cn - 1, (Bn, Tn), generator=g)
    hotc = torch.where(torch.rand(Bn, Tn, generator=g) < p_blank, torch.full_like(hotc, Cn - 1), hotc)
    x.scatter_add_(2, hotc.unsqueeze(-1), torch.full((Bn, Tn, 1), float(hot)))
    return torch.log_softmax(x, -1)


def frame_counts(chunks, lens):
    """a chunking of the frame axis as per-feed, per-stream frame counts"""
    out, s = [], 0
    for n in chunks:
        out.append([min(max(l - s, 0), n) for l in lens])
        s += n
    return out


def feed_counts(stream, x, counts, cursors=None):
    """feeds x (B, T, C) to `stream`, feed k giving stream b its next counts[k][b] frames; returns the last feed's outputs"""
    Bn = x.shape[0]
    cur = [0] * Bn if cursors is None else cursors
    out = None
    for cnt in counts:
        tc = max(max(cnt), 1)
        buf = torch.zeros(Bn, tc, x.shape[2], device=x.device)
        for b in range(Bn):
            buf[b, :cnt[b]] = x[b, cur[b]:cur[b] + cnt[b]]
            cur[b] += cnt[b]
        out = stream.feed(buf, cnt)
    return out


def one_shot(x, lens, W, k, cp, n_best, lm=None, bank=None):
    from lightning_asr_amd import ops
    lt = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=x.device)
    blank = x.shape[-1] - 1
    if bank is not None:
        return ops.ctc_beam_decode_biased(x, lt, blank, bank, W, k, cp, n_best, lm)
    if lm is not None:
        return ops.ctc_beam_decode_lm(x, lt, blank, lm, W, k, cp, n_best)
    return ops.ctc_beam_decode(x, lt, blank, W, k, cp, n_best)


def open_stream(x, W, k, cp, n_best, t_cap, lm=None, bank=None):
    from lightning_asr_amd import ops
    return ops.CtcBeamStream(x.shape[0], x.shape[2], x.shape[2] - 1, W, k, cp, n_best, t_cap, lm=lm, bank=bank, device=x.device)


def assert_same(got, want, what):
    """got: a stream's outputs (tokens of pitch t_cap); want: the one-shot outputs of n frames (tokens of pitch n)"""
    torch.cuda.synchronize()
    assert len(got) == len(want), what
    n = want[0].shape[2]
    assert torch.equal(got[0][:, :, :n], want[0]), what
    assert (got[0][:, :, n:] == -1).all(), what
    for i in range(1, len(want)):
        assert torch.equal(got[i], want[i]), (what, i)


@pytest.fixture(scope="module")
def x28(dev):
    return peaky(B, T, C, 3).to(dev).contiguous()


@pytest.fixture(scope="module")
def lms(tmp_path_factory):
    d = tmp_path_factory.mktemp("stream_lm")
    return {"char": S.write_arpa(d / "en3.arpa", EN, 3, 400, seed=3), "word": S.write_arpa(d / "w3.arpa", WORDS, 3, 400, seed=3)}


def hot_bank(dev, x, lens):
    """phrases cut from the unbiased best hypothesis of stream 0 (matched, and one whose match stays unfinished) and a few more"""
    from lightning_asr_amd import ops
    tok, n, _ = one_shot(x, lens, 16, 40, 1.0, 1)
    best = [int(c) for c in tok[0, 0, :int(n[0, 0])].cpu()]
    assert len(best) >= 8, best
    other = (best[6] + 1) % (x.shape[2] - 1)
    phrases = [best[1:4], best[1:3], best[-3:] + [other], best[4:6] + [other], [5, 9], [2]]
    weights = [2.0, 1.0, 3.0, 1.5, 2.0, 0.5]
    return ops.build_hotwords(phrases, weights, n_classes=x.shape[2], blank=x.shape[2] - 1, device=dev)


# ------------------------------------------------------------------------------------------------ the plain search
@pytest.mark.parametrize("W", [1, 4, 16, 128])
@pytest.mark.parametrize("k", [40, 8])
@pytest.mark.parametrize("cp", [1.0, 0.95])
def test_stream_equals_one_shot(dev, x28, W, k, cp):
    n_best = min(W, 4)
    want = one_shot(x28, LENS, W, k, cp, n_best)
    st = open_stream(x28, W, k, cp, n_best, T)
    plans = {name: frame_counts(ch, LENS) for name, ch in FRAME_CHUNKS.items()}
    plans["ragged_idle"] = RAGGED
    for name, counts in plans.items():
        st.reset()
        got = feed_counts(st, x28, counts)
        assert_same(got, want, name)
        assert st.frames.tolist() == LENS and st.dropped.tolist() == [0, 0, 0], name


def test_idle_feed_keeps_state_and_rewrites_outputs(dev, x28):
    st = open_stream(x28, 16, 40, 1.0, 4, T)
    feed_counts(st, x28, [[30, 30, 0]])
    before = [t.clone() for t in (st.tokens, st.n_tokens, st.scores)]
    st.tokens.fill_(7); st.n_tokens.fill_(7); st.scores.fill_(7.0)
    got = st.feed(torch.zeros(B, 3, C, device=dev), [0, 0, 0])
    torch.cuda.synchronize()
    for u, v in zip(got, before):
        assert torch.equal(u, v)
    got = feed_counts(st, x28, [[31, 7, 0]], cursors=[30, 30, 0])
    assert_same(got, one_shot(x28, LENS, 16, 40, 1.0, 4), "after an idle feed")


# ------------------------------------------------------------------------------------------------ every scorer
def scorer_case(dev, kind, x28, lms):
    """(x, lens, lm, bank) of one scorer kind"""
    from lightning_asr_amd import ops
    if kind == "wlm":
        xs, _ = WS.sentence_logp(WVOCAB, WORDS, B, T, 7)
        x = xs.to(dev).contiguous()
        return x, LENS, ops.load_arpa(lms["word"], WVOCAB, dev, 0.8, 1.0), None
    lm = ops.load_arpa(lms["char"], EN, dev, 0.7, 1.5) if kind in ("lm", "lm_bias") else None     # beta 1.5: the early cutoff works
    bank = hot_bank(dev, x28, LENS) if kind in ("bias", "lm_bias") else None
    return x28, LENS, lm, bank


@pytest.mark.parametrize("kind", ["lm", "wlm", "bias", "lm_bias"])
def test_stream_equals_one_shot_with_scorer(dev, x28, lms, kind):
    x, lens, lm, bank = scorer_case(dev, kind, x28, lms)
    W, n_best = 16, 4
    k = 40 if kind != "wlm" else 6
    want = one_shot(x, lens, W, k, 1.0, n_best, lm, bank)
    assert len(want) == (5 if bank is not None else 4)
    if kind == "wlm":
        assert not lm.is_character_based()
    assert int(want[1][0, 0]) > 0                                # the best hypothesis of stream 0 has labels
    if bank is not None:
        assert (want[4][0] != 0).any()                           # and the bank credited some hypothesis of stream 0
    st = open_stream(x, W, k, 1.0, n_best, T, lm, bank)
    for name, counts in (("uneven", frame_counts(FRAME_CHUNKS["uneven"], lens)), ("ragged_idle", RAGGED)):
        st.reset()
        assert_same(feed_counts(st, x, counts), want, (kind, name))


@pytest.mark.parametrize("kind", ["wlm", "bias"])
def test_prefix_property(dev, x28, lms, kind):
    """after the frames [0, n) the outputs are the one-shot decode of those n frames alone, every end term included"""
    x, lens, lm, bank = scorer_case(dev, kind, x28, lms)
    W, n_best = 16, 4
    k = 40 if kind != "wlm" else 6
    st = open_stream(x, W, k, 1.0, n_best, T, lm, bank)
    s = 0
    for cut in (23, 40):
        got = feed_counts(st, x, frame_counts([cut - s], [max(l - s, 0) for l in lens]), cursors=[s] * B)
        want = one_shot(x[:, :cut].contiguous(), [min(l, cut) for l in lens], W, k, 1.0, n_best, lm, bank)
        assert_same(got, want, (kind, cut))
        s = cut


def test_large_vocabulary(dev):
    Bn, Tn, Cn, W = 2, 40, 4334, 8
    x = peaky(Bn, Tn, Cn, 11).to(dev).contiguous()
    lens = [40, 29]
    want = one_shot(x, lens, W, 40, 1.0, 4)
    st = open_stream(x, W, 40, 1.0, 4, Tn)
    assert_same(feed_counts(st, x, frame_counts([7, 1, 32], lens)), want, "C = 4334")


def test_widest_candidate_set(dev):
    Bn, Tn, Cn, W = 2, 30, 80, 128
    x = peaky(Bn, Tn, Cn, 12, hot=3.0).to(dev).contiguous()       # flat rows: all 64 kept classes stay finite candidates
    lens = [30, 17]
    want = one_shot(x, lens, W, 64, 1.0, 4)
    st = open_stream(x, W, 64, 1.0, 4, Tn)
    assert_same(feed_counts(st, x, frame_counts([4, 13, 1, 12], lens)), want, "W = 128, cutoff_top_n = 64")


# ------------------------------------------------------------------------------------------------ reset, capacity, capture
def test_reset_of_one_stream_in_mid_feed(dev, x28):
    lens = [61, 37, 30]
    W, n_best = 16, 4
    want = one_shot(x28, lens, W, 40, 1.0, n_best)
    st = open_stream(x28, W, 40, 1.0, n_best, T)
    feed_counts(st, x28, [[20, 20, 20]])
    st.reset(rows=[1])
    torch.cuda.synchronize()
    assert st.frames.tolist() == [20, 0, 20]
    # stream 1 starts over from its first frame; 0 and 2 go on where they were
    got = feed_counts(st, x28, [[11, 30, 10], [30, 7, 0]], cursors=[20, 0, 20])
    assert_same(got, want, "reset(rows=[1])")
    assert st.frames.tolist() == lens


def test_capacity_clamp_and_host_check(dev, x28):
    from lightning_asr_amd import _lib, ops
    W, n_best, cap = 16, 4, 20
    want = one_shot(x28[:, :cap].contiguous(), None, W, 40, 1.0, n_best)
    st = open_stream(x28, W, 40, 1.0, n_best, cap)
    # through the C entry point, past the Python object's own check: 12 + 18 frames into a stream of 20
    nb = int(_lib.load().lasr_ctc_beam_stream_workspace_bytes(B, 18, C, W, 40))
    ws = ops._ws(nb, dev)
    chunks = [x28[:, s:e].contiguous() for s, e in ((0, 12), (12, 30))]
    for chunk in chunks:
        _lib.call("lasr_ctc_beam_stream_feed", chunk.data_ptr(), None, B, chunk.shape[1], C, C - 1, W, 40, 1.0, n_best,
                  _lib.C.byref(st._scorer), st._state.data_ptr(), st._state_bytes, cap, st.tokens.data_ptr(), st.n_tokens.data_ptr(),
                  st.scores.data_ptr(), st._n_frames.data_ptr(), st._n_dropped.data_ptr(), ws.data_ptr(), nb,
                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st.frames.tolist() == [20, 20, 20] and st.dropped.tolist() == [10, 10, 10]
    assert_same((st.tokens, st.n_tokens, st.scores), want, "T_cap = 20")
    # the Python object refuses such a feed before launching anything
    st2 = open_stream(x28, W, 40, 1.0, n_best, cap)
    st2.feed(x28[:, :12].contiguous())
    with pytest.raises(ValueError):
        st2.feed(x28[:, 12:30].contiguous())
    torch.cuda.synchronize()
    assert st2.frames.tolist() == [12, 12, 12] and st2.dropped.tolist() == [0, 0, 0]
    got = st2.feed(x28[:, 12:20].contiguous())
    assert_same(got, want, "exactly t_cap frames")


def test_graph_capture_replay_advances_the_state(dev, x28):
    W, n_best, step = 16, 4, 10
    want = one_shot(x28, LENS, W, 40, 0.95, n_best)
    st = open_stream(x28, W, 40, 0.95, n_best, T)
    buf = torch.zeros(B, step, C, device=dev)
    lens = torch.zeros(B, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        st.feed(buf, lens)                                       # warm-up: the workspace is allocated outside the capture
    torch.cuda.current_stream().wait_stream(side)
    st.reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = st.feed(buf, lens)
    for s in range(0, T, step):
        n = min(step, T - s)
        buf.zero_()
        buf[:, :n] = x28[:, s:s + n]
        lens.copy_(torch.tensor([min(max(l - s, 0), n) for l in LENS], dtype=torch.int32))
        g.replay()
    assert_same(got, want, "graph replay")
    assert st.frames.tolist() == LENS


# ------------------------------------------------------------------------------------------------ greedy
def test_greedy_stream_equals_greedy_decode(dev):
    from lightning_asr_amd import ops
    blank = C - 1
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, C, (B, T), generator=g).to(torch.int32)
    ids[torch.rand(B, T, generator=g) < 0.4] = blank
    # "uneven" cuts at 5, 6 and 23: a label run across 5 and 6, a blank run across 23, equal labels split by a blank at 6
    ids[0, 3:8] = 4
    ids[0, 20:26] = blank
    ids[1, 4] = 9; ids[1, 5] = blank; ids[1, 6] = 9
    ids[1, 21:24] = 2
    ids = ids.to(dev).contiguous()
    lens = [61, 37, 0]
    tok, n = ops.greedy_decode(ids, torch.tensor(lens, dtype=torch.int32, device=dev), blank)
    plans = {name: frame_counts(ch, lens) for name, ch in FRAME_CHUNKS.items()}
    plans["ragged_idle"] = RAGGED
    st = ops.GreedyStream(B, blank, T, device=dev)
    for name, counts in plans.items():
        st.reset()
        cur = [0] * B
        for cnt in counts:
            tc = max(max(cnt), 1)
            buf = torch.full((B, tc), blank, dtype=torch.int32, device=dev)
            for b in range(B):
                buf[b, :cnt[b]] = ids[b, cur[b]:cur[b] + cnt[b]]
                cur[b] += cnt[b]
            got_tok, got_n = st.feed(buf, cnt)
        torch.cuda.synchronize()
        assert torch.equal(got_n, n), name
        for b in range(B):
            assert torch.equal(got_tok[b, :int(n[b])], tok[b, :int(n[b])]), (name, b)
            assert (got_tok[b, int(n[b]):] == -1).all(), (name, b)
        assert st.frames.tolist() == lens
