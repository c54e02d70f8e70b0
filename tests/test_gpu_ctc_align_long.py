"""GPU tier of long-recording forced alignment (csrc/ctc_align_long.hip).  The banded recursion is a max and one f32 add per
state per frame and the band rule is integer arithmetic on an argmax with a fixed tie rule, so the kernel is held BIT FOR BIT to
ops.ctc_align where the band covers the lattice, and to the numpy oracle (tests/helpers/ctc_align_long_oracle.py) where it does
not: score, frame states, frame log-probs, label spans, status and the band origins.  Then guard bands round every output and
the workspace, graph capture, and the argument checks."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import ctc_align_long_oracle as L  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("score", "frame_state", "frame_logp", "label_start", "label_end", "status", "band_lo")
PLANTED = [(600, 250, 3, 28), (700, 600, 4, 28), (900, 400, 1, 28), (2001, 1000, 3, 28), (700, 300, 4, 4334), (1300, 640, 3, 28)]
ALL_BANDS = list(range(256, 4097, 256)) + [5120, 6144, 7168, 8192]       # every wave count of both forms

_planted = {}
_want = {}


def planted(T, S, C, hot, seed=0):
    """one planted recording per shape, made once and never written to"""
    key = (T, S, C, hot, seed)
    if key not in _planted:
        lp, lab = L.planted(T, S, C, hot, seed)
        lp.setflags(write=False)
        _planted[key] = (lp, lab)
    return _planted[key]


def oracle(key, lp, targets, in_lens, tgt_lens, blank, band):
    if (key, band) not in _want:
        _want[(key, band)] = L.align_long_batch(lp, targets, in_lens, tgt_lens, blank, band)
    return _want[(key, band)]


def run_ops(dev, lp, targets, in_lens, tgt_lens, blank, band):
    from lightning_asr_amd import ops
    out = ops.ctc_align_long(torch.tensor(lp, device=dev), torch.from_numpy(np.asarray(targets, np.int64)).to(dev),
                             None if in_lens is None else torch.from_numpy(np.asarray(in_lens, np.int32)).to(dev),
                             torch.from_numpy(np.asarray(tgt_lens, np.int32)).to(dev), blank, band)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def assert_exact(got, want, ctx):
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (ctx, name, g.shape, w.shape, g.dtype, w.dtype)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError("%s: %s differs at %d places, first %s: got %r want %r"
                                 % (ctx, name, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


def assert_band_consistent(got, in_lens, band):
    """band_lo never falls, is a multiple of G, changes only at multiples of R, and holds every frame's state"""
    R, G = L.R, L.G
    st, lo = got[1], got[6]
    for b in range(st.shape[0]):
        Tb = int(in_lens[b])
        assert (lo[b, Tb:] == -1).all()
        l = lo[b, :Tb].astype(np.int64)
        if Tb == 0:
            continue
        assert l[0] == 0 and (l % G == 0).all() and (np.diff(l) >= 0).all()
        assert ((np.nonzero(np.diff(l))[0] + 1) % R == 0).all()
        if got[5][b] == 0:
            s = st[b, :Tb]
            assert ((s >= l) & (s < l + band)).all()


# ------------------------------------------------------------------------------------------------ wide band == ops.ctc_align
@pytest.mark.parametrize("S,T,C", [(0, 1, 28), (1, 2, 28), (127, 501, 28), (600, 2001, 28), (2047, 2001, 28), (256, 501, 4334)])
def test_wide_band_equals_ctc_align(dev, S, T, C):
    """band >= 2S+1: the band never moves and the result is the full lattice's"""
    from lightning_asr_amd import ops
    B = 3
    rng = np.random.RandomState(S + T)
    lp = torch.log_softmax(torch.from_numpy(rng.standard_normal((B, T, C)).astype(np.float32)) * 2.0, -1).to(dev).contiguous()
    targets = rng.randint(0, min(C - 1, 4), size=(B, S)).astype(np.int64)          # a small alphabet: runs of equal labels
    in_lens = np.array([T, max(T - 1, 1), T // 2], np.int32)
    tgt_lens = np.array([S, S // 2, S], np.int32)                                  # row 2 is short of frames when S is large
    tg, il, tl = torch.from_numpy(targets).to(dev), torch.from_numpy(in_lens).to(dev), torch.from_numpy(tgt_lens).to(dev)
    band = next(w for w in ALL_BANDS if w >= 2 * S + 1)
    want = ops.ctc_align(lp, tg, il, tl, C - 1)
    for w in (band, 4096):
        got = ops.ctc_align_long(lp, tg, il, tl, C - 1, band=w)
        torch.cuda.synchronize()
        for name, g, x in zip(NAMES, got[:5], want):
            assert torch.equal(g, x), (S, T, C, w, name)
        feasible = torch.isfinite(want.score)
        assert torch.equal(got.status == 0, feasible), (got.status, want.score)
        lo = got.band_lo.cpu().numpy()
        for b in range(B):
            assert (lo[b, :in_lens[b]] == 0).all() and (lo[b, in_lens[b]:] == -1).all()


# ------------------------------------------------------------------------------------------------ banded == oracle
@pytest.mark.parametrize("band", [256, 512, 1024])
@pytest.mark.parametrize("T,S,hot,C", PLANTED)
def test_planted_matches_oracle(dev, T, S, hot, C, band):
    lp, lab = planted(T, S, C, hot)
    want = oracle(("planted", T, S, C, hot), lp[None], lab[None], None, [S], C - 1, band)
    assert want[5][0] == 0
    got = run_ops(dev, lp[None], lab[None], None, [S], C - 1, band)
    assert_exact(got, want, (T, S, hot, C, band))
    assert_band_consistent(got, [T], band)


@pytest.mark.parametrize("T,S,band", [(6100, 3000, 1024), (10001, 5000, 4096), (10001, 5000, 8192)])
def test_above_the_old_label_cap(dev, T, S, band):
    """S above LASR_CTC_MAX_LABELS; W = 4096 is four waves of 16 states per lane, 8192 the eight-wave form"""
    lp, lab = planted(T, S, 28, 3)
    want = oracle(("planted", T, S, 28, 3), lp[None], lab[None], None, [S], 27, band)
    assert want[5][0] == 0 and want[6][0].max() > 0                                # the band did move
    got = run_ops(dev, lp[None], lab[None], None, [S], 27, band)
    assert_exact(got, want, (T, S, band))
    assert_band_consistent(got, [T], band)


@pytest.mark.parametrize("band", ALL_BANDS)
def test_every_wave_count(dev, band):
    """a planted recording through every band the kernel takes: 1..16 waves of 4 states per lane, 1..8 of 16; the recording is
    long enough for the band to move"""
    T, S, C = (3001, 1400, 28) if band < 2801 else (10001, 5000, 28)
    lp, lab = planted(T, S, C, 3)
    want = oracle(("planted", T, S, C, 3), lp[None], lab[None], None, [S], C - 1, band)
    assert want[5][0] == 0 and want[6][0].max() > 0
    got = run_ops(dev, lp[None], lab[None], None, [S], C - 1, band)
    assert_exact(got, want, band)


def test_plain_random_banded_differs_from_full(dev):
    """nothing planted: the band prunes, and the kernel prunes exactly as the definition does"""
    import ctc_align_oracle as A
    T, S, C, band = 801, 380, 28, 256
    rng = np.random.RandomState(3)
    lp = L.log_softmax(rng.standard_normal((T, C)).astype(np.float32) * 2.0)
    lab = rng.randint(0, C - 1, size=S).astype(np.int64)
    want = oracle(("plain", T, S), lp[None], lab[None], None, [S], C - 1, band)
    full = A.align_batch(lp[None], lab[None], None, [S], C - 1)
    assert not np.array_equal(want[1], full[1])                                    # banded != full on these inputs
    assert_exact(run_ops(dev, lp[None], lab[None], None, [S], C - 1, band), want, "plain")


@pytest.mark.parametrize("T,S", [(1, 0), (2, 1), (31, 12), (32, 12), (33, 12), (47, 20), (48, 20), (49, 20), (97, 40), (385, 190)])
def test_short_rows_and_chunk_borders(dev, T, S):
    """T around the period R = 32, the backtrace chunk (8 rows) and its prefetch depth (48 rows), and the 64-frame flush"""
    lp, lab = planted(T, S, 28, 2, seed=T)
    want = oracle(("planted", T, S, 28, 2, T), lp[None], lab[None], None, [S], 27, 256)
    assert_exact(run_ops(dev, lp[None], lab[None], None, [S], 27, 256), want, (T, S))


def ragged_case():
    """B = 4: a feasible full row, a row short of frames (status 1), a row without frames, a feasible shorter row"""
    T, S_max, C = 900, 400, 28
    rng = np.random.RandomState(11)
    lp = L.log_softmax(rng.standard_normal((4 * T, C)).astype(np.float32)).reshape(4, T, C).copy()
    targets = rng.randint(0, C - 1, size=(4, S_max)).astype(np.int64)
    in_lens = np.array([T, 300, 0, 700], np.int32)
    tgt_lens = np.array([S_max, S_max, 5, 300], np.int32)
    for b in (0, 3):
        p, lab = L.planted(int(in_lens[b]), int(tgt_lens[b]), C, 3, 20 + b)
        lp[b, :in_lens[b]] = p
        targets[b, :tgt_lens[b]] = lab
    return lp, targets, in_lens, tgt_lens


@pytest.mark.parametrize("band", [256, 1024])
def test_ragged_batch_with_infeasible_rows(dev, band):
    lp, targets, in_lens, tgt_lens = ragged_case()
    want = oracle("ragged", lp, targets, in_lens, tgt_lens, 27, band)
    assert want[5].tolist() == [0, 1, 1, 0]
    got = run_ops(dev, lp, targets, in_lens, tgt_lens, 27, band)
    assert_exact(got, want, ("ragged", band))
    assert_band_consistent(got, in_lens, band)
    for b in (1, 2):
        assert got[0][b] == -np.inf and (got[1][b] == -1).all() and (got[2][b] == 0).all() and (got[3][b] == -1).all()


@pytest.mark.parametrize("band,status", [(256, 2), (512, 0), (1024, 0)])
def test_lost_case(dev, band, status):
    """the band loses the path at W = 256, keeps a worse one at 512 and is the full lattice at 1024"""
    import ctc_align_oracle as A
    lp, lab = L.lost_case()
    want = oracle("lost", lp[None], lab[None], None, [300], 27, band)
    full = A.align_batch(lp[None], lab[None], None, [300], 27)
    assert want[5][0] == status
    if band == 512:
        assert want[0][0] < full[0][0]
    if band == 1024:
        assert all(np.array_equal(w, f) for w, f in zip(want[:5], full))
    got = run_ops(dev, lp[None], lab[None], None, [300], 27, band)
    assert_exact(got, want, ("lost", band))
    if status == 2:
        assert got[0][0] == -np.inf and (got[1] == -1).all() and (got[3] == -1).all() and (got[6][0] >= 0).all()


def test_tight_row_needs_reach(dev):
    lp, lab = L.tight_case()
    want = oracle("tight", lp[None], lab[None], None, [400], 27, 256)
    assert want[5][0] == 0 and want[6][0, -1] == 576
    assert_exact(run_ops(dev, lp[None], lab[None], None, [400], 27, 256), want, "tight")


# ------------------------------------------------------------------------------------------------ guards, capture, arguments
@pytest.mark.parametrize("band", [256, 768, 2048])
def test_guard_bands(dev, band):
    """every output and the workspace sit between sentinel regions that must come back intact"""
    from lightning_asr_amd import _lib
    G = 1024
    lp_h, targets, in_lens, tgt_lens = ragged_case()
    B, T, C = lp_h.shape
    S_max = targets.shape[1]
    lp = torch.from_numpy(lp_h).to(dev)
    tg, il, tl = torch.from_numpy(targets).to(dev), torch.from_numpy(in_lens).to(dev), torch.from_numpy(tgt_lens).to(dev)
    nb = int(_lib.load().lasr_ctc_align_long_workspace_bytes(B, T, S_max, band))
    assert nb == B * T * band // 4 and nb % 256 == 0
    sizes = {"score": B, "frame_state": B * T, "frame_logp": B * T, "label_start": B * S_max, "label_end": B * S_max, "status": B,
             "band_lo": B * T, "ws": nb // 4}
    bufs = {k: torch.full((n + 2 * G,), -12345, dtype=torch.int32, device=dev) for k, n in sizes.items()}
    ptr = {k: v.data_ptr() + 4 * G for k, v in bufs.items()}
    _lib.call("lasr_ctc_align_long", lp.data_ptr(), tg.data_ptr(), il.data_ptr(), tl.data_ptr(), B, T, C, S_max, C - 1, band, ptr["score"],
              ptr["frame_state"], ptr["frame_logp"], ptr["label_start"], ptr["label_end"], ptr["status"], ptr["band_lo"], ptr["ws"], nb,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for k, v in bufs.items():
        h = v.cpu().numpy()
        assert (h[:G] == -12345).all() and (h[G + sizes[k]:] == -12345).all(), (band, k)
    body = {k: bufs[k].cpu().numpy()[G:G + sizes[k]] for k in sizes}
    got = (body["score"].view(np.float32), body["frame_state"].reshape(B, T), body["frame_logp"].view(np.float32).reshape(B, T),
           body["label_start"].reshape(B, S_max), body["label_end"].reshape(B, S_max), body["status"], body["band_lo"].reshape(B, T))
    assert_exact(got, oracle("ragged", lp_h, targets, in_lens, tgt_lens, C - 1, band), ("guard", band))
    assert_band_consistent(got, in_lens, band)


def test_deterministic_and_graph_capture(dev):
    from lightning_asr_amd import ops
    lp_h, targets, in_lens, tgt_lens = ragged_case()
    lp = torch.from_numpy(lp_h).to(dev)
    tg, il, tl = torch.from_numpy(targets).to(dev), torch.from_numpy(in_lens).to(dev), torch.from_numpy(tgt_lens).to(dev)
    for band in (256, 1024):
        a = ops.ctc_align_long(lp, tg, il, tl, 27, band=band)
        b = ops.ctc_align_long(lp, tg, il, tl, 27, band=band)
        torch.cuda.synchronize()
        for u, v in zip(a, b):
            assert torch.equal(u, v)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            ops.ctc_align_long(lp, tg, il, tl, 27, band=band)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            c = ops.ctc_align_long(lp, tg, il, tl, 27, band=band)
        for _ in range(2):
            for o in c:
                o.fill_(-7)
            g.replay()
            torch.cuda.synchronize()
            for u, v in zip(a, c):
                assert torch.equal(u, v)


def test_argument_errors(dev):
    from lightning_asr_amd import _lib, ops
    assert ops.ctc_align_long_period() == L.R and ops.ctc_align_long_granule() == L.G
    B, T, C, S = 1, 40, 28, 6
    lp = torch.log_softmax(torch.randn(B, T, C, generator=torch.Generator().manual_seed(0)), -1).to(dev)
    tg = torch.arange(S, dtype=torch.int64, device=dev).unsqueeze(0)
    tl = torch.tensor([S], dtype=torch.int32, device=dev)
    out = ops.ctc_align_long(lp, tg, None, tl, C - 1, band=256)
    assert int(out.status[0]) == 0
    for band in (0, 128, 300, 4352, 8192 + 1024):
        assert _lib.load().lasr_ctc_align_long_workspace_bytes(B, T, S, band) == 0
        with pytest.raises(ValueError, match="band"):
            ops.ctc_align_long(lp, tg, None, tl, C - 1, band=band)
    with pytest.raises(ValueError, match="blank"):
        ops.ctc_align_long(lp, tg.clone().fill_(C - 1), None, tl, C - 1, band=256)
    nb = int(_lib.load().lasr_ctc_align_long_workspace_bytes(B, T, S, 256))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    outs = [o.data_ptr() for o in out]

    def raw(logp=lp.data_ptr(), blank=C - 1, band=256, status=outs[5], ws_bytes=nb, c=C):
        _lib.call("lasr_ctc_align_long", logp, tg.data_ptr(), None, tl.data_ptr(), B, T, c, S, blank, band, outs[0], outs[1], outs[2], outs[3],
                  outs[4], status, outs[6], ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream)
    raw()
    with pytest.raises(_lib.LasrError, match=r"\(-1\)"):          # LASR_E_ARG
        raw(logp=None)
    with pytest.raises(_lib.LasrError, match=r"\(-1\)"):
        raw(status=None)
    for kw in ({"band": 300}, {"band": 0}, {"band": 16384}, {"blank": C}, {"blank": -1}, {"c": 1}):
        with pytest.raises(_lib.LasrError, match=r"\(-2\)"):      # LASR_E_SHAPE
            raw(**kw)
    with pytest.raises(_lib.LasrError, match=r"\(-3\)"):          # LASR_E_WORKSPACE
        raw(ws_bytes=nb - 1)
    torch.cuda.synchronize()
