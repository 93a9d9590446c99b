"""GPU: the exact top-k selection behind the indexer scores (csrc/topk_select.hip) against plain torch on the CPU.

One reference, `check_rows`, for every case. For row b with window w = score[b, rs : rs + len]:
  1. the returned raw indices are distinct and lie in [0, len);
  2. their values, sorted, equal torch.sort(w, descending=True).values[:topk] exactly;
  3. of the indices whose value equals the k-th value, the returned ones are the lowest.
len <= topk is compared slot by slot (0 .. len - 1, then -1). Mapped outputs are compared as sorted rows with the mapping
applied to the raw set on the CPU; page tables are random permutations."""
import pytest
import torch

pytestmark = pytest.mark.gpu
K = 2048


def check_rows(score, raw, lengths, row_starts=None, topk=K):
    score, raw = score.cpu(), raw.cpu()
    assert raw.dtype == torch.int32 and tuple(raw.shape) == (score.shape[0], topk)
    for b in range(score.shape[0]):
        n, rs = int(lengths[b]), int(row_starts[b]) if row_starts is not None else 0
        r = raw[b].long()
        if n <= topk:
            want = torch.cat([torch.arange(max(n, 0)), torch.full((topk - max(n, 0),), -1)])
            assert torch.equal(r, want), f"row {b} (len {n})"
            continue
        w = score[b, rs:rs + n]
        assert int(r.min()) >= 0 and int(r.max()) < n and r.unique().numel() == topk, f"row {b}: indices"
        top = torch.sort(w, descending=True).values[:topk]
        assert torch.equal(torch.sort(w[r], descending=True).values, top), f"row {b}: values"
        ties = (w == top[-1]).nonzero().flatten()
        got = torch.sort(r[w[r] == top[-1]]).values
        assert torch.equal(got, ties[:got.numel()]), f"row {b}: ties"


def rows_equal(got, want):
    assert torch.equal(torch.sort(got.cpu().long(), dim=1).values, torch.sort(want.cpu().long(), dim=1).values)


def i32(x, dev):
    return torch.as_tensor(x, dtype=torch.int32, device=dev)


def two_valued(n, n_hi):
    x = torch.zeros(n)
    x[torch.randperm(n)[:n_hi]] = 1.5
    return x


ROWS = {  # name -> row of 40000 (each overflows the candidate list or stresses one digit)
    "all_equal": lambda n: torch.full((n,), 0.37),
    "shared_leading_bits": lambda n: 1 + 2.0 ** -20 * torch.randint(0, 8, (n,)),
    "two_values_2047": lambda n: two_valued(n, 2047),
    "two_values_2049": lambda n: two_valued(n, 2049),
    "relu_few_positives": lambda n: torch.where(torch.rand(n) < 0.03, torch.rand(n), torch.zeros(n)),
    "relu_half_zeros": lambda n: torch.randn(n).clamp(min=0),
    "integers": lambda n: torch.randint(0, 50, (n,)).float(),
    "negative": lambda n: -torch.rand(n) - 0.5,
    "infinities": lambda n: torch.randn(n).masked_fill(torch.rand(n) < 0.01, float("inf")).masked_fill(torch.rand(n) < 0.01, float("-inf")),
    "above_fp16": lambda n: torch.rand(n) * 1e6 + 65504,
    "normal": lambda n: torch.randn(n),
}


@pytest.mark.parametrize("name", sorted(ROWS))
def test_row_kinds(sglk, dev, name):
    torch.manual_seed(1)
    score = torch.stack([ROWS[name](40000), ROWS[name](40000)])
    lengths = [40000, 4000]  # one row through the histogram passes over the row, one straight into the candidate list
    check_rows(score, sglk.fast_topk_v2(score.to(dev), i32(lengths, dev), K), lengths)


def test_path_boundary_and_determinism(sglk, dev):
    torch.manual_seed(2)
    lengths = [0, 1, 2047, 2048, 2049, -3, 4096, 4097]
    score = torch.randint(0, 200, (len(lengths), 4100)).float().to(dev)
    a = sglk.fast_topk_v2(score, i32(lengths, dev), K)
    check_rows(score, a, lengths)
    assert torch.equal(a, sglk.fast_topk_v2(score, i32(lengths, dev), K))


def test_misaligned_windows(sglk, dev):
    torch.manual_seed(3)
    width = 20001 + 7
    score = torch.randn(4, width + 13, device=dev)[:, :width]  # row stride larger than the width
    assert score.stride(0) > score.shape[1]
    starts, lengths = [7, 1, 2, width - 4099], [20001, 4099, 20001, 4099]  # 7 = 3 mod 4; row 0 and row 3 end at the last column
    check_rows(score, sglk.fast_topk_v2(score, i32(lengths, dev), K, i32(starts, dev)), lengths, starts)


@pytest.mark.parametrize("with_starts", [False, True])
@pytest.mark.parametrize("form", ["decode", "prefill", "ragged"])
def test_transforms(sglk, dev, form, with_starts):
    torch.manual_seed(4)
    cu = [0, 3, 4, 9, 11]  # uneven, a sequence of one token, a last sequence
    B, L = cu[-1], 6000
    score = torch.randn(B, L, device=dev)
    starts = [int(x) for x in torch.randint(0, 900, (B,))] if with_starts else None
    lengths = [int(x) for x in torch.randint(2049, 5000, (B,))]
    lengths[2], lengths[5] = 100, 2048
    st = i32(starts, dev) if with_starts else None
    raw = sglk.fast_topk_v2(score, i32(lengths, dev), K, st)
    check_rows(score, raw, lengths, starts)
    raw = raw.cpu().long()
    if form == "ragged":
        off = torch.randint(0, 10 ** 6, (B,))
        got = sglk.fast_topk_transform_ragged_fused(score, i32(lengths, dev), i32(off, dev), K, st)
        want = raw + off[:, None]
    else:
        if form == "decode":  # a table row per score row (with row_starts it is still found through cu_seqlens_q)
            cu = list(range(B + 1))
        table = torch.stack([torch.randperm(L) for _ in range(len(cu) - 1)])
        got = sglk.fast_topk_transform_fused(score, i32(lengths, dev), i32(table, dev), i32(cu, dev), K, st)
        seq = torch.bucketize(torch.arange(B), torch.tensor(cu), right=True) - 1
        want = table[seq[:, None], raw.clamp(min=0)]
    rows_equal(got, torch.where(raw >= 0, want, -1))
    for b in (2, 5):  # len <= topk: slot by slot
        assert torch.equal(got[b].cpu().long(), torch.where(raw[b] >= 0, want[b], -1))


@pytest.mark.parametrize("v2", [False, True])
@pytest.mark.parametrize("page_size", [1, 64])
@pytest.mark.parametrize("topk", [1, 512, 1000, 2048])
def test_topk_transform_512(sglk, dev, topk, page_size, v2):
    torch.manual_seed(5)
    B, L = 3, 5120
    score = torch.randn(B, L, device=dev)
    lengths = [L, 2500, min(topk, 700)]
    pages = torch.randperm(B * L // page_size).view(B, L // page_size)
    out = torch.empty(B, topk, dtype=torch.int32, device=dev)
    raw = torch.empty_like(out) if v2 == (page_size == 1) else None  # with and without the raw output, over both ops
    args = (score, i32(lengths, dev).view(B, 1), i32(pages, dev), out, page_size)
    if v2:
        sglk.topk_transform_512_v2(*args, torch.empty(4, dtype=torch.int32, device=dev), raw)
    else:
        sglk.topk_transform_512(*args, raw)
    if raw is None:
        raw = torch.empty_like(out)
        sglk.topk_transform_512(*args, raw)
    check_rows(score, raw, lengths, topk=topk)
    p = raw.cpu().long()
    want = pages[torch.arange(B)[:, None], p.clamp(min=0) // page_size] * page_size + p.clamp(min=0) % page_size
    rows_equal(out, torch.where(p >= 0, want, -1))


def test_graph_capture(sglk, dev):
    torch.manual_seed(6)
    score = torch.randn(4, 9000, device=dev)
    lengths, off = i32([9000, 5000, 2049, 30], dev), i32([0, 10, 20, 30], dev)
    eager = sglk.fast_topk_transform_ragged_fused(score, lengths, off, K)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            out = sglk.fast_topk_transform_ragged_fused(score, lengths, off, K)
    torch.cuda.current_stream().wait_stream(side)
    g.replay()
    assert torch.equal(out, eager)
    score.copy_(torch.randint(0, 9, (4, 9000)).float())
    for _ in range(2):
        g.replay()
        assert torch.equal(out, sglk.fast_topk_transform_ragged_fused(score, lengths, off, K))
    check_rows(score, out - off[:, None] * (out >= 0), [9000, 5000, 2049, 30])


def test_argument_errors(sglk, dev):
    score, lengths = torch.zeros(2, 4096, device=dev), i32([4096, 4096], dev)
    with pytest.raises(ValueError):
        sglk.fast_topk_v2(score, lengths, 1024)
    with pytest.raises(ValueError):
        sglk.fast_topk_transform_ragged_fused(score[0], lengths, lengths, K)
    with pytest.raises(RuntimeError, match="Float32"):
        sglk.fast_topk_v2(score.half(), lengths, K)
    with pytest.raises(RuntimeError, match="Int32"):
        sglk.fast_topk_v2(score, lengths.long(), K)
    with pytest.raises(RuntimeError, match="elements"):
        sglk.fast_topk_v2(score, lengths[:1], K)
    with pytest.raises(RuntimeError, match="topk"):
        sglk.topk_transform_512(score, lengths, torch.zeros(2, 4096, dtype=torch.int32, device=dev),
                                torch.empty(2, 4096, dtype=torch.int32, device=dev), 1)
