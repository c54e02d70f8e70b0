"""The bf16 GEMM tiles on v_mfma_f32_16x16x32_bf16: every tile form at ragged M, N and K, all four operand layouts,
through the epilogues whose index mapping follows the accumulator layout (bias, row mask, BN column sums, f32 slabs).
Small-integer operands keep every product and partial sum exact, so results are compared bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _ref(A, Bm, tA, tB):
    return (A.t() if tA else A).double() @ (Bm if tB else Bm.t()).double()


# 256-row tile: narrow (N <= 256, 256 x 128 tiles) and wide (256 x 256), every layout, K tails off the 64- and 8-grid
@pytest.mark.parametrize("M,N,K", [(16001, 200, 136), (15999, 520, 200), (9000, 776, 72), (16032, 256, 329)])
@pytest.mark.parametrize("tA,tB", [(False, False), (False, True), (True, False), (True, True)])
def test_big_tile_layouts_epilogue_exact(dev, M, N, K, tA, tB):
    from lightning_asr_amd import ops
    g = torch.Generator().manual_seed(M + 3 * N + 7 * K + 11 * tA + 13 * tB)
    if tA and M > 10000:
        M = 8003                            # keep the [K][M] operand of the transposed-A forms small
    if K % 8 and (tA or tB):
        K += 8 - K % 8                      # row-contiguous operands: the aligned (16-byte) path of the model
    A = torch.randint(-2, 3, (K, M) if tA else (M, K), generator=g).float()
    Bm = (torch.rand((K, N) if tB else (N, K), generator=g) < 0.05).float()
    bias = torch.randint(-3, 4, (N,), generator=g).float()
    ref = _ref(A, Bm, tA, tB) + bias.double()
    assert ref.abs().max() <= 256
    got, _ = ops.gemm(A.bfloat16().to(dev), Bm.bfloat16().to(dev), M, N, K, tA, tB, bias=bias.to(dev))
    assert torch.equal(got.cpu().double(), ref)
    # row mask and column statistics (sequences of T rows, some cut short, one empty)
    T = 501
    B = M // T
    Mm = B * T
    lens = torch.randint(0, T + 1, (B,), generator=g).to(torch.int32)
    lens[0], lens[-1] = T, 0
    keep = (torch.arange(T).view(1, T) < lens.view(B, 1)).view(Mm, 1).double()
    Am = A[:, :Mm] if tA else A[:Mm]
    if tA:
        Am = Am.contiguous()
    refm = (_ref(Am, Bm, tA, tB) + bias.double()) * keep
    got, stats = ops.gemm(Am.bfloat16().to(dev), Bm.bfloat16().to(dev), Mm, N, K, tA, tB, bias=bias.to(dev), row_lens=lens.to(dev),
                          rows_per_seq=T, want_stats=True)
    assert torch.equal(got.cpu().double(), refm)
    # f32 partial sums: exact for the sums, the sums of squares can pass 2^24
    assert torch.allclose(stats[:N].cpu().double(), refm.sum(0), rtol=1e-6, atol=0)
    assert torch.allclose(stats[N:].cpu().double(), (refm * refm).sum(0), rtol=1e-6, atol=0)


# 128 x 128 tile (small problems): bf16 with bias, and f32 split-K slabs, every layout
@pytest.mark.parametrize("M,N,K", [(333, 200, 136), (97, 77, 515), (1000, 264, 40)])
@pytest.mark.parametrize("tA,tB", [(False, False), (False, True), (True, False), (True, True)])
def test_small_tile_layouts_exact(dev, M, N, K, tA, tB):
    from lightning_asr_amd import ops
    g = torch.Generator().manual_seed(M * 5 + N + K + 2 * tA + tB)
    A = torch.randint(-3, 4, (K, M) if tA else (M, K), generator=g).float()
    Bm = torch.randint(-2, 3, (K, N) if tB else (N, K), generator=g).float()
    bias = torch.randint(-3, 4, (N,), generator=g).float()
    ref = _ref(A, Bm, tA, tB)
    got, _ = ops.gemm(A.bfloat16().to(dev), Bm.bfloat16().to(dev), M, N, K, tA, tB, out_dtype=torch.float32, split_k=3)
    assert torch.equal(got.cpu().double(), ref)
    got, _ = ops.gemm(A.bfloat16().to(dev), Bm.bfloat16().to(dev), M, N, K, tA, tB, out_dtype=torch.float32, bias=bias.to(dev))
    assert torch.equal(got.cpu().double(), ref + bias.double())
    if (ref + bias.double()).abs().max() <= 256:
        got, _ = ops.gemm(A.bfloat16().to(dev), Bm.bfloat16().to(dev), M, N, K, tA, tB, bias=bias.to(dev))
        assert torch.equal(got.cpu().double(), ref + bias.double())


def test_wgrad_multi_ragged_exact(dev):
    """Split-K slab form of the 256-row tile (stage weight gradients): ragged rows (K of the product) and ragged channel counts."""
    from lightning_asr_amd import ops
    g = torch.Generator().manual_seed(17)
    rows = 7001
    shapes = [(520, 264), (136, 200), (256, 512), (72, 776)]
    dys = [torch.randint(-2, 3, (rows, co), generator=g).float() for co, _ in shapes]
    xs = [(torch.rand(rows, ci, generator=g) < 0.05).float() * torch.randint(-1, 2, (rows, ci), generator=g).float() for _, ci in shapes]
    for split in (1, 5):
        outs = ops.wgrad_multi([d.bfloat16().to(dev) for d in dys], [x.bfloat16().to(dev) for x in xs], split_k=split)
        for d, x, o in zip(dys, xs, outs):
            assert torch.equal(o.cpu(), d.t() @ x)
