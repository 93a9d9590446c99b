"""GPU parity: fp8_mqa_logits / fp8_paged_mqa_logits / fp8_paged_mqa_logits_triton (csrc/mqa_logits.hip) against a float64
evaluation of   logits[i, j] = k_scale[j] * sum_h w[i, h] * relu(q[i, h, :] . k[j, :])   inside the window, 0 outside.

Shapes straddle the kernels' constants: 32 keys = one MFMA fragment (Nk 1, 33), KT = 128 keys = a ring stage of the
ragged kernel and the smallest key chunk of a paged workgroup (129 = KT + 1, 257 = 2 KT + 1: at these sizes the host gives
every workgroup one tile / one fragment a wave, so they straddle workgroup edges), QB = 16 queries a ragged workgroup
(Nq 1, 17), 32 heads = one M-fragment (H 4: a partly filled one, 33: the second one with one head, 64). The two
*_ring_steady_state tests are sized so that the host picks several tiles / fragments per workgroup: the rings' loops.

The bound inside the window is derived, not measured: products of two e4m3 values are exact in fp32, a result takes at
most 128 + 64 fp32 additions of at most 2^-23 relative each - doubled for margin - and relu is 1-Lipschitz, so
|out - ref| <= 2^-14 * A with A the same formula on |q|, |k|, |w| without the relu. Outside the window: exactly 0."""
import pytest
import torch

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
D, KT, QB = 128, 128, 16


def reference(q, k, k_scale, w, ks, ke):
    """float64, on the inputs' device; q (Nq, H, D) and k (Nk, D), or one key list (Nq, Nk, D) and scale row per query;
    e4m3 or its uint8 bytes -> (logits, bound A, window mask)"""
    qd, kd, sc = q.view(FP8).double(), k.view(FP8).double(), k_scale.double()
    eq, sc = ("ihd,ijd->ihj", sc) if kd.dim() == 3 else ("ihd,jd->ihj", sc[None])
    out = (torch.einsum(eq, qd, kd).clamp_(min=0) * w.double()[:, :, None]).sum(1) * sc
    A = (torch.einsum(eq, qd.abs(), kd.abs()) * w.double().abs()[:, :, None]).sum(1) * sc.abs()
    j = torch.arange(k.shape[-2], device=k.device)[None]
    mask = (j >= ks[:, None]) & (j < ke[:, None])
    return out * mask, A, mask


def make_case(Nq, Nk, H, seed, known=False):
    """q, k, k_scale, w: random full-range e4m3 / signed weights / scales in [0.5, 1.5), or (known) small integers,
    asymmetric in i, h, j, d, with power-of-two scales: every partial sum is an integer below 2^24"""
    if known:
        i, h, d = torch.arange(Nq).view(-1, 1, 1), torch.arange(H).view(1, -1, 1), torch.arange(D).view(1, 1, -1)
        j = torch.arange(Nk).view(-1, 1)
        q = (((3 * i + 5 * h + d + d // 32) % 7) - 3).float().to(FP8)
        k = (((2 * j + 3 * d.view(1, -1) + d.view(1, -1) // 16) % 5) - 2).float().to(FP8)
        w = (((i + 2 * h) % 5) - 2).view(Nq, H).float()
        return q, k, 2.0 ** ((j.view(-1) % 3) - 1).float(), w
    g = torch.Generator().manual_seed(seed)
    q = ((torch.rand(Nq, H, D, generator=g) - 0.5) * 2 * 448).to(FP8)
    k = ((torch.rand(Nk, D, generator=g) - 0.5) * 2 * 448).to(FP8)
    return q, k, torch.rand(Nk, generator=g) + 0.5, torch.randn(Nq, H, generator=g)


def windows(Nq, Nk):
    """One query: a window that starts and ends inside 32-key fragments (and leaves the last tile of three unseen).
    Otherwise a causal staircase of 7 keys a query - the first block of 16 never sees a key from 112 on, so with Nk > KT whole
    tiles are invisible to it: the skip path - with a window inside one fragment, an empty row, ke < ks, and a last
    query (the second block's, with Nq = 17) that sees everything through bounds that need clamping."""
    if Nq == 1:
        return torch.tensor([Nk // 3], dtype=torch.int32), torch.tensor([Nk - Nk // 4], dtype=torch.int32)
    ks = torch.zeros(Nq, dtype=torch.int32)
    ke = torch.tensor([min(Nk, 7 * (i + 1)) for i in range(Nq)], dtype=torch.int32)
    ks[1], ke[1] = 3, min(Nk, 20)
    ks[2], ke[2] = 5, 5
    ks[3], ke[3] = 9, 2
    ks[-1], ke[-1] = -2, Nk + 5
    return ks, ke


def check(out, ref, A, mask):
    assert torch.equal(out[~mask], torch.zeros_like(out[~mask]))
    err = (out.double() - ref).abs()
    worst = (err / A.clamp(min=1e-300))[mask].max().item() if mask.any() else 0.0
    print("worst |out - ref| / A = %.3g (bound %.3g)" % (worst, 2.0 ** -14))
    assert bool((err <= 2.0 ** -14 * A)[mask].all())


@pytest.mark.parametrize("dtype", [torch.uint8, FP8], ids=["u8", "e4m3"])
@pytest.mark.parametrize("H", [4, 33, 64])
@pytest.mark.parametrize("Nq", [1, QB + 1])
@pytest.mark.parametrize("Nk", [1, 33, KT + 1, 2 * KT + 1])
def test_ragged_parity(sglk, dev, Nk, Nq, H, dtype):
    q, k, k_scale, w = make_case(Nq, Nk, H, seed=Nk + Nq + H)
    ks, ke = windows(Nq, Nk)
    out = sglk.fp8_mqa_logits(q.view(dtype).to(dev), (k.view(dtype).to(dev), k_scale.to(dev)), w.to(dev), ks.to(dev), ke.to(dev))
    assert out.shape == (Nq, Nk) and out.dtype == torch.float32
    check(out.cpu(), *reference(q, k, k_scale, w, ks, ke))


def slots(table, page_size, max_seq_len, block):
    """byte offsets (B, max_seq_len) of every position's key row and scale in the cache, by the layout's formula"""
    j = torch.arange(max_seq_len, device=table.device)
    pb, t = table[:, j // page_size].long() * (page_size * (D + 4)), j % page_size
    ko = pb + t * D if block else pb + t * (D + 4)
    return ko, (pb + page_size * D + t * 4 if block else ko + D)


def make_paged(B, H, page_size, seq_lens, max_seq_len, block, seed, known=False):
    """-> (q, cache, w, table): keys and scales of make_case scattered into a paged cache through a shuffled table whose
    padding entries are valid pages too. Unused bytes of the cache hold 0x38 (1.0 in e4m3)."""
    g = torch.Generator().manual_seed(seed)
    cols = (max_seq_len + page_size - 1) // page_size
    num_pages = B * cols + 3
    table = torch.randperm(num_pages, generator=g)[:B * cols].view(B, cols).to(torch.int32)
    cache = torch.full((num_pages, page_size, 1, D + 4), 0x38, dtype=torch.uint8)
    q, k, k_scale, w = make_case(B, B * max_seq_len, H, seed, known)
    ko, so = slots(table, page_size, max_seq_len, block)
    live = torch.arange(max_seq_len)[None] < torch.tensor(seq_lens)[:, None]
    cache.view(-1)[ko[live][:, None] + torch.arange(D)] = k.view(torch.uint8).view(B, max_seq_len, D)[live]
    cache.view(-1)[so[live][:, None] + torch.arange(4)] = k_scale.view(torch.uint8).view(B, max_seq_len, 4)[live]
    return q, cache, w, table


def paged_reference(q, cache, w, table, seq_lens, max_seq_len, block):
    """gathers every key row and scale from the cache (on its device), then the float64 reference with windows [0, seq_len)"""
    dv = cache.device
    ko, so = slots(table.to(dv), cache.shape[1], max_seq_len, block)
    k = cache.view(-1)[ko[:, :, None] + torch.arange(D, device=dv)]
    sc = cache.view(-1)[so[:, :, None] + torch.arange(4, device=dv)].view(torch.float32).squeeze(-1)
    sl = torch.tensor(seq_lens, device=dv)
    return reference(q.to(dv), k, sc, w.to(dv), torch.zeros_like(sl), sl)


@pytest.mark.parametrize("H", [4, 64])
@pytest.mark.parametrize("page_size", [1, 4, 64])
@pytest.mark.parametrize("block", [False, True], ids=["row", "block"])
def test_paged_parity(sglk, dev, block, page_size, H):
    """seq_lens: empty, one key, two pages and a bit, KT + 1 = one more than a workgroup's key chunk; max_seq_len beyond all.
    The 3-D query with (B, 1) seq_lens must give what the 4-D call gives."""
    seq_lens, max_seq_len = [0, 1, 2 * page_size + 3, KT + 1], KT + 71
    q, cache, w, table = make_paged(4, H, page_size, seq_lens, max_seq_len, block, seed=page_size)
    fn = sglk.fp8_paged_mqa_logits_triton if block else sglk.fp8_paged_mqa_logits
    sl = torch.tensor(seq_lens, dtype=torch.int32, device=dev)
    args = (cache.to(dev), w.to(dev))
    tab = torch.cat([table, table], 1).to(dev)[:, :table.shape[1]]  # a strided view: row stride twice the columns
    out = fn(q.view(torch.uint8).to(dev).unsqueeze(1), *args, sl, tab, None, max_seq_len)
    assert out.shape == (4, max_seq_len) and out.dtype == torch.float32
    check(out.cpu(), *paged_reference(q, cache, w, table, seq_lens, max_seq_len, block))
    if page_size == 4:
        assert torch.equal(fn(q.to(dev), *args, sl.view(-1, 1), tab, None, max_seq_len, clean_logits=True), out)


def test_ragged_ring_steady_state(sglk, dev):
    """The host gives a ragged workgroup up to 16 tiles, halved while query blocks x chunks < 2 x 256 CUs: the shapes above
    all run one tile a workgroup. 2 query blocks over 2049 tiles make it 8 (2 x 257 >= 512), so the ring wraps, the counted
    waits of tiles 1 and >= 2 run, and n_k % 4 == 0 takes the 16-byte zero fill. Query i of the first block sees 450 keys
    from 300 + 700 i: its hull starts and ends inside chunks (zero fill on both sides of live tiles) and every wave meets
    unseen tiles between seen ones; the last query sees every key. Reference in float64 on the device."""
    Nq, Nk, H = QB + 1, 2048 * KT + 4, 64
    q, k, k_scale, w = (t.to(dev) for t in make_case(Nq, Nk, H, seed=7))
    ks = torch.tensor([300 + 700 * i for i in range(Nq)], dtype=torch.int32, device=dev)
    ke = ks + 450
    ks[-1], ke[-1] = -2, Nk + 5
    check(sglk.fp8_mqa_logits(q, (k, k_scale), w, ks, ke), *reference(q, k, k_scale, w, ks, ke))


@pytest.mark.parametrize("block", [False, True], ids=["row", "block"])
def test_paged_ring_steady_state(sglk, dev, block):
    """A paged workgroup's chunk is 2048 keys, halved while batch x chunks < 4 x 256 CUs: 4 x 131072 positions give 512,
    four fragments a wave, so all three ring slots and the reloads of slots 0 and 1 run. Sequences end inside a chunk,
    on a chunk's edge, at one key and at none."""
    seq_lens, max_seq_len = [256 * 512, 70003, 1, 0], 256 * 512
    q, cache, w, table = make_paged(4, 64, 64, seq_lens, max_seq_len, block, seed=9)
    fn = sglk.fp8_paged_mqa_logits_triton if block else sglk.fp8_paged_mqa_logits
    out = fn(q.to(dev), cache.to(dev), w.to(dev), torch.tensor(seq_lens, dtype=torch.int32, device=dev), table.to(dev), None, max_seq_len)
    check(out, *paged_reference(q, cache.to(dev), w, table, seq_lens, max_seq_len, block))


def test_known_answer_ragged(sglk, dev):
    """exact integers: a transposed fragment, a swapped K half, a wrong lane-half exchange or a neighbour's weight shows"""
    Nq, Nk, H = QB + 1, KT + 33, 64
    q, k, k_scale, w = make_case(Nq, Nk, H, 0, known=True)
    ks, ke = windows(Nq, Nk)
    ref, A, _ = reference(q, k, k_scale, w, ks, ke)
    assert A.max() < 2 ** 24 and ref.abs().max() > 0
    out = sglk.fp8_mqa_logits(q.to(dev), (k.to(dev), k_scale.to(dev)), w.to(dev), ks.to(dev), ke.to(dev))
    assert torch.equal(out.cpu().double(), ref)


@pytest.mark.parametrize("block", [False, True], ids=["row", "block"])
def test_known_answer_paged(sglk, dev, block):
    seq_lens, max_seq_len, page_size = [KT + 3, 0, 40], KT + 10, 4
    q, cache, w, table = make_paged(3, 33, page_size, seq_lens, max_seq_len, block, seed=1, known=True)
    ref, A, _ = paged_reference(q, cache, w, table, seq_lens, max_seq_len, block)
    assert A.max() < 2 ** 24 and ref.abs().max() > 0
    fn = sglk.fp8_paged_mqa_logits_triton if block else sglk.fp8_paged_mqa_logits
    out = fn(q.to(dev).unsqueeze(1), cache.to(dev), w.to(dev), torch.tensor(seq_lens, dtype=torch.int32, device=dev),
             table.to(dev), None, max_seq_len)
    assert torch.equal(out.cpu().double(), ref)


@pytest.mark.parametrize("paged", [False, True], ids=["ragged", "paged"])
def test_graph_replay_matches_eager(sglk, dev, paged):
    if paged:
        seq_lens, max_seq_len = [0, 1, KT + 1, 70], KT + 71
        q, cache, w, table = make_paged(4, 64, 64, seq_lens, max_seq_len, False, seed=3)
        args = (q.to(dev), cache.to(dev), w.to(dev), torch.tensor(seq_lens, dtype=torch.int32, device=dev), table.to(dev),
                None, max_seq_len)
        fn = sglk.fp8_paged_mqa_logits
    else:
        q, k, k_scale, w = make_case(QB + 1, 2 * KT + 1, 64, seed=4)
        ks, ke = windows(QB + 1, 2 * KT + 1)
        args = (q.to(dev), (k.to(dev), k_scale.to(dev)), w.to(dev), ks.to(dev), ke.to(dev))
        fn = sglk.fp8_mqa_logits
    eager = fn(*args).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = fn(*args)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        out.fill_(3.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


@pytest.mark.parametrize("what", ["D=64", "H=65", "q second dim 2", "fp16 weights", "int64 ks", "cache row D+8", "strided cache"])
def test_errors(sglk, dev, what):
    Dq, H = (64 if what == "D=64" else D), (65 if what == "H=65" else 4)
    z = lambda *shape, dtype=torch.uint8: torch.zeros(*shape, dtype=dtype, device=dev)  # noqa: E731
    wdt = torch.float16 if what == "fp16 weights" else torch.float32
    with pytest.raises((RuntimeError, ValueError)):
        if what in ("q second dim 2", "cache row D+8", "strided cache"):
            q = z(2, 2 if what == "q second dim 2" else 1, H, Dq)
            cache = z(4, 4, 1, D + (8 if what == "cache row D+8" else 4))
            cache = cache if what != "strided cache" else z(4, 8, 1, D + 4)[:, ::2]
            sglk.fp8_paged_mqa_logits(q, cache, z(2, H, dtype=wdt), z(2, dtype=torch.int32), z(2, 2, dtype=torch.int32), None, 8)
        else:
            idt = torch.int64 if what == "int64 ks" else torch.int32
            sglk.fp8_mqa_logits(z(2, H, Dq), (z(3, Dq), z(3, dtype=torch.float32)), z(2, H, dtype=wdt), z(2, dtype=idt), z(2, dtype=idt))
