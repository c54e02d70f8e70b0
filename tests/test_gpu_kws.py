"""GPU tier of CTC keyword search (csrc/ctc_kws.hip).  The recursion is a selection and one f32 add per state per frame on
emissions that are one f32 subtraction, so the kernel is held to the numpy oracle (tests/helpers/kws_oracle.py) BIT FOR BIT:
hit counts, spans, scores, best scores and best spans - integers equal, scores by torch.equal - across both state layouts (one
state per lane up to 32 labels, two above) and their edge, both emission forms (rows staged in LDS, global gather) and the
switch between them, ragged lengths, phrases with repeats, phrases longer than the clip, exact ties, planted occurrences and
more hits than slots."""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import kws_oracle as K  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("n_hits", "hit_span", "hit_score", "best_score", "best_span")

# The emission rows of an utterance are staged in LDS while (T + 2) * C * 4 bytes of rows (a pad row on either side), the T row
# maxima (rounded up to 16 bytes) and 2 KB of headroom fit the 160 KB of a CU, and C % 4 == 0.  For C = 28 that is
# 112 (T + 2) + 4 T + 2048 <= 163840: T <= 1392.  One frame more and the walk gathers from global memory.
LDS_MAX_T_C28 = 1392


def cyc(n, first):
    """n labels without an adjacent repeat"""
    return [(first + i) % 26 for i in range(n)]


# L = 1, 2, 32 | 33, 64 (the two state layouts and their edge), repeats ("aa", "abab", "aab"), and a duplicate: K = 9 is more than
# the eight waves of one workgroup
PHRASES = [[3], [3, 7], cyc(32, 0), cyc(33, 5), cyc(64, 2), [0, 0], [0, 1, 0, 1], [0, 0, 1], [3, 7]]


def plain(B, T, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn(B, T, C, generator=g) * 2.0, -1).numpy()


def grid(B, T, C, seed):
    """multiples of 2^-10: every partial sum is exact, so different paths tie exactly"""
    return (np.round(plain(B, T, C, seed) * 1024.0) / 1024.0).astype(np.float32)


def peaky_path(paths, C):
    """one class at log 0.92 per frame (the path's), the rest equal: e = 0 along the path, one constant off it"""
    paths = np.asarray(paths)
    lp = np.full(paths.shape + (C,), math.log(0.08 / (C - 1)), np.float32)
    np.put_along_axis(lp, paths[..., None], np.float32(math.log(0.92)), axis=-1)
    return lp


def peaky(B, T, C, seed):
    """greedy paths of short runs over a few labels and the blank: the short phrases ("d", "dh", "aa", "abab", "aab") occur in
    them here and there with score 0, in runs of frames with e = 0 that the earliest-start and latest-end rules have to resolve"""
    rng = np.random.RandomState(seed)
    alphabet = [0, 0, 0, 1, 1, 3, 7, C - 1, C - 1, C - 1]
    paths = np.zeros((B, T), np.int64)
    for b in range(B):
        t = 0
        while t < T:
            n = int(rng.randint(1, 4))
            paths[b, t:t + n] = alphabet[int(rng.randint(len(alphabet)))]
            t += n
    return peaky_path(paths, C)


GENS = {"plain": plain, "grid": grid, "peaky": peaky}


@functools.lru_cache(maxsize=None)
def case(gen, B, T, C, lens, phrases_key, threshold, max_hits):
    """inputs and the oracle's outputs, computed once and shared (read-only)"""
    phrases = [list(p) for p in phrases_key]
    lp = GENS[gen](B, T, C, 11 + T + C)
    lp.setflags(write=False)
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in phrases])])
    want = K.search_batch(lp, None if lens is None else list(lens), C - 1, [c for p in phrases for c in p], offsets,
                          max(len(p) for p in phrases), threshold, max_hits)
    return lp, phrases, want


def key(phrases):
    return tuple(tuple(p) for p in phrases)


def run_ops(dev, lp, lens, phrases, blank, threshold, max_hits):
    from lightning_asr_amd import ops
    bank = ops.build_keywords(phrases, n_classes=lp.shape[-1], blank=blank, device=dev)
    out = ops.ctc_keyword_search(torch.from_numpy(np.array(lp)).to(dev), None if lens is None else
                                 torch.tensor(list(lens), dtype=torch.int32, device=dev), blank, bank, threshold, max_hits)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def assert_exact(got, want, ctx):
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (ctx, name, g.shape, w.shape, g.dtype, w.dtype)
        same = torch.equal(torch.from_numpy(g), torch.from_numpy(w)) if g.dtype == np.float32 else np.array_equal(g, w)
        if not same:
            bad = np.argwhere(g != w)
            raise AssertionError("%s: %s differs at %d places, first %s: got %r want %r"
                                 % (ctx, name, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


@pytest.mark.parametrize("lens", [(40, 17, 0), None])
@pytest.mark.parametrize("gen,threshold", [("plain", -5.0), ("grid", -5.0), ("peaky", -0.5), ("peaky", -3.0)])
def test_kws_matches_oracle_c28(dev, gen, threshold, lens):
    """B = 3, T = 40, C = 28 (rows in LDS), K = 9: every phrase form at once, ragged and full lengths"""
    B, T, C = 3, 40, 28
    lp, phrases, want = case(gen, B, T, C, lens, key(PHRASES), threshold, 8)
    n_hits, _, _, best, bspan = want
    assert not np.isfinite(best[:, 4]).any() and (bspan[:, 4] == -1).all()          # 64 labels on at most 40 frames: dead
    assert np.isfinite(best[0, :4]).all()                                            # 32 and 33 labels fit 40 frames
    if lens is not None:
        assert not np.isfinite(best[1, 2:5]).any() and not np.isfinite(best[2]).any()   # 17 frames, no frame
        assert (n_hits[2] == 0).all()
    assert n_hits.max() >= 2
    if gen == "plain":
        assert n_hits.max() > 8                                                      # more hits than slots occurs
    if gen == "peaky":
        assert (want[2][want[1][..., 0] >= 0] == 0).any()                            # exact occurrences: score 0
    assert np.array_equal(want[0][:, 1], want[0][:, 8]) and np.array_equal(want[1][:, 1], want[1][:, 8])   # the duplicate
    assert_exact(run_ops(dev, lp, lens, phrases, C - 1, threshold, 8), want, (gen, threshold, lens))


@pytest.mark.parametrize("gen", ["grid", "peaky"])
def test_kws_single_keyword(dev, gen):
    """K = 1: one wave of the workgroup walks, the others only stage"""
    B, T, C = 2, 33, 28
    for phrase in ([0, 1, 0, 1], cyc(33, 1)):                      # 33 labels on exactly 33 frames: one path, every frame used
        lp, phrases, want = case(gen, B, T, C, (33, 20), key([phrase]), -4.0, 4)
        assert_exact(run_ops(dev, lp, (33, 20), phrases, C - 1, -4.0, 4), want, (gen, len(phrase)))
    assert np.isfinite(want[3][0, 0]) and want[4][0, 0].tolist() == [0, 33] and want[3][1, 0] == -np.inf


@pytest.mark.parametrize("gen", ["plain", "peaky"])
def test_kws_global_gather_c4336(dev, gen):
    """C = 4336: a multiple of 4 whose rows do not fit LDS (24 frames are 451 KB): row maxima from the pre-pass, gather ahead"""
    B, T, C = 2, 24, 4336
    phrases = [[3], [4000, 7], [0, 0], [0, 1, 0, 1], cyc(20, 3), [c * 150 for c in cyc(24, 0)], cyc(33, 0)]
    thr = -8.0 if gen == "plain" else -0.5
    lp, phrases, want = case(gen, B, T, C, (24, 9), key(phrases), thr, 4)
    assert np.isfinite(want[3][0, :6]).all() and want[3][0, 6] == -np.inf
    assert_exact(run_ops(dev, lp, (24, 9), phrases, C - 1, thr, 4), want, gen)


def test_kws_both_sides_of_the_lds_switch(dev):
    """C = 28 at T = LDS_MAX_T_C28 (the longest clip whose rows are staged) and one frame more (global gather): the same answers
    as the oracle on both sides, past a thousand frames of recursion"""
    C = 28
    phrases = [[3], [0, 1, 0, 1, 3], cyc(33, 0)]
    for T in (LDS_MAX_T_C28, LDS_MAX_T_C28 + 1):
        assert ((T + 2) * C * 4 + (T * 4 + 15) // 16 * 16 + 2048 <= 160 * 1024) == (T == LDS_MAX_T_C28)
        lp, ph, want = case("peaky", 1, T, C, None, key(phrases), -3.0, 8)
        assert want[0][0, 0] > 8 and want[0][0, 1] >= 1
        assert_exact(run_ops(dev, lp, None, ph, C - 1, -3.0, 8), want, T)


def test_kws_no_lds_switch_in_a_fresh_process(dev, tmp_path):
    """LASR_CTC_NO_LDS=1 (read once per process, so a child): the C = 28 case through the global-gather form"""
    B, T, C, lens = 3, 40, 28, (40, 17, 0)
    lp, phrases, want = case("grid", B, T, C, lens, key(PHRASES), -5.0, 8)
    np.savez(tmp_path / "in.npz", lp=lp, lens=np.array(lens, np.int32), labels=np.array([c for p in phrases for c in p], np.int64),
             sizes=np.array([len(p) for p in phrases], np.int64))
    code = ("import sys, numpy as np, torch; sys.path.insert(0, %r); from lightning_asr_amd import ops\n"
            "d = np.load(sys.argv[1]); cuts = np.cumsum(d['sizes'])[:-1]\n"
            "phrases = [p.tolist() for p in np.split(d['labels'], cuts)]\n"
            "bank = ops.build_keywords(phrases, n_classes=28, blank=27, device='cuda')\n"
            "out = ops.ctc_keyword_search(torch.from_numpy(d['lp']).cuda(), torch.from_numpy(d['lens']).cuda(), 27, bank, -5.0, 8)\n"
            "torch.cuda.synchronize(); np.savez(sys.argv[2], *[o.cpu().numpy() for o in out])\n" % ROOT)
    env = dict(os.environ, LASR_CTC_NO_LDS="1")
    subprocess.run([sys.executable, "-c", code, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], check=True, env=env, timeout=300)
    got = np.load(tmp_path / "out.npz")
    assert_exact(tuple(got["arr_%d" % i] for i in range(5)), want, "LASR_CTC_NO_LDS")


def planted(C, T, places, phrase_frames):
    """a greedy path of blanks with `phrase_frames` (the classes of an occurrence, frame by frame) at each of `places`"""
    path = np.full((1, T), C - 1, np.int64)
    for t0 in places:
        path[0, t0:t0 + len(phrase_frames)] = phrase_frames
    return peaky_path(path, C)


@pytest.mark.parametrize("C", [5, 28])
def test_kws_planted_occurrences(dev, C):
    """the phrase sits on the greedy path at two known places.  threshold -0.5 with L = 7: thr = -3.5, and one off-path frame
    costs log((0.08 / (C - 1)) / 0.92) = -3.83 (C = 5; -5.74 for C = 28), so only exact occurrences pass: the hits are exactly
    the planted spans with score 0"""
    blank = C - 1
    phrase = [0, 1, 2, 3, 0, 1, 2]
    first = [0, 0, 1, blank, 2, 2, 3, 0, blank, 1, 1, 2, 2]                  # 13 frames: [5, 18)
    second = [0, 1, 2, 3, 3, 0, 1, 2, 2]                                     # 9 frames: [24, 33)
    assert K.collapse(first, blank) == phrase and K.collapse(second, blank) == phrase
    T = 40
    path = np.full((1, T), blank, np.int64)
    path[0, 5:18], path[0, 24:33] = first, second
    lp = peaky_path(path, C)
    assert math.log((0.08 / (C - 1)) / 0.92) < -3.5
    want = K.search_batch(lp, None, blank, phrase, [0, 7], 7, -0.5, 4)
    assert want[0][0, 0] == 2 and want[1][0, 0, :2].tolist() == [[5, 18], [24, 33]] and want[2][0, 0].tolist() == [0.0] * 4
    got = run_ops(dev, lp, None, [phrase], blank, -0.5, 4)
    assert got[0][0, 0] == 2 and got[1][0, 0].tolist() == [[5, 18], [24, 33], [-1, -1], [-1, -1]] and got[2][0, 0].tolist() == [0.0] * 4
    assert got[3][0, 0] == 0.0 and got[4][0, 0].tolist() == [24, 33]          # the best: the latest of the tied ends
    assert_exact(got, want, ("planted", C))


def test_kws_more_hits_than_slots_and_guard_bands(dev):
    """max_hits = 1 with three occurrences: n_hits == 3, slot 0 holds the first, and nothing is written outside the outputs: each
    lies inside a larger poisoned tensor that must come back intact, as must the workspace's surroundings"""
    from lightning_asr_amd import _lib
    G, POISON = 256, -12345
    for C, B in [(28, 2), (4336, 1)]:
        blank, T, Kn = C - 1, 36, 3
        occ = [0, 0, 1, blank, 1]                                            # "abb"
        lp = np.concatenate([planted(C, T, (2, 14, 29), occ)] * B)
        phrases = [[0, 1, 1], [1], [0, 1, 0]]
        want = K.search_batch(lp, None, blank, [c for p in phrases for c in p], [0, 3, 4, 7], 3, -0.5, 1)
        assert want[0][0].tolist() == [3, 6, 0] and want[1][0, 0, 0].tolist() == [2, 7]     # "b": its two runs in each occurrence
        nb = int(_lib.load().lasr_ctc_kws_workspace_bytes(B, T, Kn))
        assert nb > 0 and nb % 4 == 0
        sizes = {"n_hits": B * Kn, "hit_span": B * Kn * 2, "hit_score": B * Kn, "best_score": B * Kn, "best_span": B * Kn * 2, "ws": nb // 4}
        bufs = {k: torch.full((n + 2 * G,), POISON, dtype=torch.int32, device=dev) for k, n in sizes.items()}
        ptr = {k: v.data_ptr() + 4 * G for k, v in bufs.items()}
        d_lp = torch.from_numpy(lp).to(dev)
        d_lab = torch.tensor([c for p in phrases for c in p], dtype=torch.int32, device=dev)
        d_off = torch.tensor([0, 3, 4, 7], dtype=torch.int32, device=dev)
        _lib.call("lasr_ctc_kws", d_lp.data_ptr(), None, B, T, C, blank, d_lab.data_ptr(), d_off.data_ptr(), Kn, 3, -0.5, 1, ptr["n_hits"],
                  ptr["hit_span"], ptr["hit_score"], ptr["best_score"], ptr["best_span"], ptr["ws"], nb, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for k, v in bufs.items():
            h = v.cpu().numpy()
            assert (h[:G] == POISON).all() and (h[G + sizes[k]:] == POISON).all(), (C, k)
        body = {k: bufs[k].cpu().numpy()[G:G + sizes[k]] for k in sizes}
        got = (body["n_hits"].reshape(B, Kn), body["hit_span"].reshape(B, Kn, 1, 2), body["hit_score"].view(np.float32).reshape(B, Kn, 1),
               body["best_score"].view(np.float32).reshape(B, Kn), body["best_span"].reshape(B, Kn, 2))
        assert_exact(got, want, ("guard", C))
        assert got[0][0, 0] == 3 and got[1][0, 0, 0].tolist() == [2, 7] and got[1][0, 2, 0].tolist() == [-1, -1]


def test_kws_device_clamps(dev):
    """an empty phrase, a phrase longer than L_max and labels outside [0, C) reach the device through the C ABI: read as the
    oracle's clamps read them, never as an out-of-bounds access"""
    from lightning_asr_amd import _lib
    B, T, C = 1, 30, 28
    lp = plain(B, T, C, 5)
    labels, offsets, L_max = [3, 99, -5, 7, 7, 0, 1, 2], [0, 0, 3, 8], 4
    want = K.search_batch(lp, [T + 100], C - 1, labels, offsets, L_max, -5.0, 4)
    d_lp = torch.from_numpy(lp).to(dev)
    d_lab, d_off = torch.tensor(labels, dtype=torch.int32, device=dev), torch.tensor(offsets, dtype=torch.int32, device=dev)
    d_len = torch.tensor([T + 100], dtype=torch.int32, device=dev)
    out = (torch.empty(B, 3, dtype=torch.int32, device=dev), torch.empty(B, 3, 4, 2, dtype=torch.int32, device=dev),
           torch.empty(B, 3, 4, device=dev), torch.empty(B, 3, device=dev), torch.empty(B, 3, 2, dtype=torch.int32, device=dev))
    nb = int(_lib.load().lasr_ctc_kws_workspace_bytes(B, T, 3))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    _lib.call("lasr_ctc_kws", d_lp.data_ptr(), d_len.data_ptr(), B, T, C, C - 1, d_lab.data_ptr(), d_off.data_ptr(), 3, L_max, -5.0, 4,
              *[o.data_ptr() for o in out], ws.data_ptr(), nb, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert_exact(tuple(o.cpu().numpy() for o in out), want, "clamps")


def test_kws_threshold_outside_its_range_is_refused(dev):
    from lightning_asr_amd import _lib, ops
    lp = torch.from_numpy(plain(1, 8, 28, 1)).to(dev)
    bank = ops.build_keywords([[1, 2]], n_classes=28, blank=27, device=dev)
    with pytest.raises(_lib.LasrError, match=r"\(-1\).*threshold"):          # LASR_E_ARG
        ops.ctc_keyword_search(lp, None, 27, bank, threshold=0.1)
    ptrs = [t.data_ptr() for t in (lp, bank.labels, bank.offsets)]
    rc = _lib.load().lasr_ctc_kws(ptrs[0], None, 1, 8, 28, 27, ptrs[1], ptrs[2], 1, 2, 0.1, 1, ptrs[0], ptrs[0], ptrs[0], ptrs[0], ptrs[0],
                                  ptrs[0], 1 << 20, None)
    assert rc == -1
    assert ops.ctc_keyword_search(lp, None, 27, bank, threshold=0.0).n_hits.shape == (1, 1)
