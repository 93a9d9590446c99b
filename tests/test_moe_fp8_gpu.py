"""GPU parity: fp8_blockwise_scaled_grouped_mm (block-scaled fp8 MoE grouped GEMM) against the CPU oracle, expert by expert.

Data and tolerances are those of the dense op (tests/test_gemm_gpu.py): full-range e4m3, scales ~1e-3. The call uses the
argument list of reference tests/test_fp8_blockwise_moe.py:145-164. One kernel serves every row count,
so there is no regime to query: both row lists below run through it."""
import pytest
import torch

from oracle import gemm as ogemm

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
FEW_ROWS = [1, 0, 3, 17, 0]        # an empty expert, a one-row expert, a 16-row block plus one
MANY_ROWS = [256, 257, 0, 1, 515]     # exact 128-row blocks, a multiple plus one, empty, one row, blocks plus a remainder


def make_case(rows, N, K, seed, gap=0, scale_mag=1e-3):
    """a, sa over all rows (gap unowned rows behind every expert), b [E, K, N] K-contiguous, sb [E, K/128, N/128], offsets"""
    g = torch.Generator().manual_seed(seed)
    E = len(rows)
    offsets = [sum(rows[:e]) + gap * e for e in range(E)]
    total = sum(rows) + gap * E
    a = ((torch.rand(total, K, generator=g) - 0.5) * 2 * 448).to(FP8)
    b = ((torch.rand(E, N, K, generator=g) - 0.5) * 2 * 448).to(FP8).transpose(1, 2)
    sa = torch.randn(total, K // 128, generator=g) * scale_mag
    sb = (torch.randn(E, N // 128, K // 128, generator=g) * scale_mag).transpose(1, 2)
    return a, b, sa, sb, offsets


def reference(a, b, sa, sb, rows, offsets, dtype, fill=0.0):
    ref = torch.full((a.shape[0], b.shape[2]), fill, dtype=dtype)
    for e, (r, o) in enumerate(zip(rows, offsets)):
        if r:
            ref[o:o + r] = ogemm.fp8_blockwise_scaled_mm(a[o:o + r], b[e], sa[o:o + r], sb[e], dtype)
    return ref


def prepare(dev, a, b, sa, sb, rows, offsets, dtype, sa_colmajor=False, fill=0.0, problem_dtype=torch.int32):
    """device tensors in the reference's layouts -> (out, the 18 arguments)"""
    E, K, N = b.shape
    out = torch.full((a.shape[0], N), fill, dtype=dtype, device=dev)
    sa_d = sa.t().contiguous().to(dev).t() if sa_colmajor else sa.to(dev)
    b_d = b.transpose(1, 2).contiguous().to(dev).transpose(1, 2)
    sb_d = sb.transpose(1, 2).contiguous().to(dev).transpose(1, 2)
    problem_sizes = torch.tensor([[r, N, K] for r in rows], dtype=problem_dtype, device=dev)
    expert_offsets = torch.tensor(offsets, dtype=torch.int32, device=dev)
    scratch = torch.empty(E, dtype=torch.int64, device=dev)  # the CUTLASS pointer / stride / layout arrays: never touched
    return out, (out, scratch, scratch, scratch, scratch, scratch, a.to(dev), b_d, sa_d, sb_d, scratch, scratch, scratch, scratch,
                 scratch, problem_sizes, expert_offsets, scratch)


def call(sglk, dev, *case, **kw):
    out, args = prepare(dev, *case, **kw)
    sglk.fp8_blockwise_scaled_grouped_mm(*args)
    return out


@pytest.mark.parametrize("sa_colmajor", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("N,K", [(128, 128), (384, 384), (640, 1152), (256, 2048)])
@pytest.mark.parametrize("rows", [FEW_ROWS, MANY_ROWS], ids=["few", "many"])
def test_parity(sglk, dev, rows, N, K, dtype, sa_colmajor):
    a, b, sa, sb, offsets = make_case(rows, N, K, seed=N + K + len(rows))
    out = call(sglk, dev, a, b, sa, sb, rows, offsets, dtype, sa_colmajor).cpu()
    ref = reference(a, b, sa, sb, rows, offsets, dtype)
    torch.testing.assert_close(out, ref, rtol=0.02, atol=1)
    torch.testing.assert_close(out.float(), ref.float(), rtol=2e-2, atol=2e-3)


def test_many_experts(sglk, dev):
    """E = 72: more than one 64-lane chunk of the expert scan"""
    rows = [i % 3 for i in range(72)]
    a, b, sa, sb, offsets = make_case(rows, 128, 256, seed=72)
    out = call(sglk, dev, a, b, sa, sb, rows, offsets, torch.bfloat16).cpu()
    ref = reference(a, b, sa, sb, rows, offsets, torch.bfloat16)
    torch.testing.assert_close(out.float(), ref.float(), rtol=2e-2, atol=2e-3)


@pytest.mark.parametrize("rows", [[3, 0, 17], [130, 1, 70]], ids=["few", "many"])
def test_offsets_are_honoured(sglk, dev, rows):
    """3 unowned rows behind every expert (the last one included): they keep the sentinel bit for bit"""
    a, b, sa, sb, offsets = make_case(rows, 384, 256, seed=5, gap=3)
    out = call(sglk, dev, a, b, sa, sb, rows, offsets, torch.bfloat16, fill=-7.5).cpu()
    ref = reference(a, b, sa, sb, rows, offsets, torch.bfloat16, fill=-7.5)
    owned = torch.zeros(a.shape[0], dtype=torch.bool)
    for r, o in zip(rows, offsets):
        owned[o:o + r] = True
    assert torch.equal(out[~owned], ref[~owned]) and (~owned).sum() == 9
    torch.testing.assert_close(out.float(), ref.float(), rtol=2e-2, atol=2e-3)


def test_lane_and_expert_map_known_answer(sglk, dev):
    """Exact small integers, asymmetric in m, n, k and e, power-of-two scales that differ per expert, K block and N block: a wrong
    expert's weights or scales, a transposed fragment or a K-half mispairing changes an exactly representable result."""
    rows, N, K = [33, 0, 130], 256, 256
    E, total = len(rows), sum(rows)
    m = torch.arange(total).view(total, 1)
    e = torch.arange(E).view(E, 1, 1)
    n = torch.arange(N).view(1, N, 1)
    k = torch.arange(K).view(1, 1, K)
    a = (((m * 7 + k.view(1, K) * 3) % 5) - 2).float()
    b = (((n * 11 + k * 5 + (k // 16) + e * 3) % 7) - 3).float().transpose(1, 2)
    sa = 2.0 ** ((m + torch.arange(K // 128).view(1, -1)) % 2).float()
    sb = 2.0 ** ((e + torch.arange(K // 128).view(1, -1, 1) + 2 * torch.arange(N // 128).view(1, 1, -1)) % 3).float()
    offsets = [0, 33, 33]
    ref = reference(a.to(FP8), b.to(FP8), sa, sb, rows, offsets, torch.float32)
    assert ref.abs().max() < 2048  # exactly representable in fp16
    out = call(sglk, dev, a.to(FP8), b.to(FP8), sa, sb, rows, offsets, torch.float16).cpu()
    assert torch.equal(out.float(), ref)


def test_graph_replay_matches_eager(sglk, dev):
    a, b, sa, sb, offsets = make_case(FEW_ROWS, 384, 384, seed=11)
    out, args = prepare(dev, a, b, sa, sb, FEW_ROWS, offsets, torch.bfloat16)
    sglk.fp8_blockwise_scaled_grouped_mm(*args)
    eager = out.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            sglk.fp8_blockwise_scaled_grouped_mm(*args)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        out.fill_(3.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


@pytest.mark.parametrize("what", ["K=192", "N=64", "fp16 a", "int64 problem_sizes"])
def test_errors(sglk, dev, what):
    N, K = (64 if what == "N=64" else 128), (192 if what == "K=192" else 128)
    rows = [2, 1]
    a = torch.zeros(3, K).to(torch.float16 if what == "fp16 a" else FP8)
    b = torch.zeros(2, N, K).to(FP8).transpose(1, 2)
    sa, sb = torch.ones(3, max(K // 128, 1)), torch.ones(2, max(K // 128, 1), max(N // 128, 1))
    with pytest.raises(RuntimeError):
        call(sglk, dev, a, b, sa, sb, rows, [0, 2], torch.bfloat16,
             problem_dtype=torch.int64 if what == "int64 problem_sizes" else torch.int32)
