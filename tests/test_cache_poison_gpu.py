"""GPU: what an op does not read must not reach its result. Every paged or length-bounded op runs twice on the same logical
inputs - once over a CLEAN cache whose unread regions hold finite random data (what the other test files use), once over a
POISONED one whose unread regions hold NaN / Inf (what a `torch.empty` pool or a recycled page may hold) - and

  (a) the two results are bit-identical (same kernel, same live data, deterministic kernels: any difference is an unread
      byte that was read into the result - a masked row loaded and multiplied by weight 0 gives 0 x NaN = NaN);
  (b) the poisoned run passes the op's own oracle comparison, with the rule and the tolerance of the op's test file
      (test_attention_gpu.check / its fp8 bounds, the MLA tolerances, test_mqa_logits_gpu.check, test_topk_gpu.check_rows);
      the oracle sees the clean logical inputs.

Poison: 16-bit caches NaN, +Inf, -Inf in turn; e4m3 0x7F (NaN); e5m2 0x7C (Inf), 0x7F (NaN) in turn; fp32 scales NaN; top-k
scores +Inf (sorts above every real score), NaN in turn. Unread regions: a sequence's last page from seq_len on, positions
in front of cache_leftpad, page-table entries past the last live page (they name one all-poison page), spare pages, cache
rows cache_batch_idx does not select, keys / scales no query's window holds, score columns outside [row_start,
row_start + len) with the stride padding. Everything poisoned lies inside the allocation and every page id is valid.
Window-masked keys inside [leftpad, seq_len) stay finite: the reference's own math gives NaN there.

Before any upload `audit` asserts on the CPU that the unread region is not empty and holds poison only, that the live
region holds none and that it equals the clean cache's: a case that poisons nothing fails."""
import math

import pytest
import torch

from oracle import attention as oa
from oracle import mla as omla
from test_attention_gpu import check, pt_seq
from test_mqa_logits_gpu import D as MQA_D
from test_mqa_logits_gpu import FP8, make_case, make_paged, paged_reference, reference, slots, windows
from test_mqa_logits_gpu import check as mqa_check
from test_topk_gpu import K, check_rows, i32, rows_equal

pytestmark = pytest.mark.gpu

RAW = {1: torch.uint8, 2: torch.int16, 4: torch.int32}


def raw(t):
    return t.view(RAW[t.element_size()])


def poison(shape, dtype):
    """a tensor of nothing but poison, alternating element by element (the cycle of three drifts against even row lengths)"""
    i = torch.arange(math.prod(shape))
    if dtype in (torch.bfloat16, torch.float16):
        p = torch.tensor([float("nan"), float("inf"), float("-inf")])[i % 3].to(dtype)
    elif dtype == torch.float8_e4m3fn:
        p = torch.full(i.shape, 0x7F, dtype=torch.uint8).view(dtype)
    elif dtype == torch.float8_e5m2:
        p = torch.tensor([0x7C, 0x7F], dtype=torch.uint8)[i % 2].view(dtype)
    else:
        assert dtype == torch.float32
        p = torch.tensor([float("inf"), float("nan")])[i % 2]
    return p.view(shape)


def with_poison(clean, unread):
    """`clean` with poison wherever `unread` (bool, broadcast against clean's shape) is set"""
    return torch.where(unread, raw(poison(clean.shape, clean.dtype)), raw(clean)).view(clean.dtype)


def audit(poisoned, clean, unread):
    u = unread.expand(clean.shape)
    assert u.any() and not u.all()
    assert not torch.isfinite(poisoned.float()[u]).any(), "finite values in the unread region"
    assert torch.isfinite(poisoned.float()[~u]).all(), "poison in the live region"
    assert torch.isfinite(clean.float()).all()
    assert torch.equal(raw(poisoned)[~u], raw(clean)[~u])


def same_bits(got, want, what):
    ne = raw(got.cpu().contiguous()) != raw(want.cpu().contiguous())
    n = int(ne.sum())
    assert n == 0, "%s: %d of %d elements differ between the clean and the poisoned run, %d of the poisoned run's are NaN" % (
        what, n, ne.numel(), int(torch.isnan(got.float()).sum()))


def paged_layout(seqs, page, width, g):
    """-> table [b, width] int32, unread [pages, page] bool, the dead page's id. Sequence i owns ceil(seq / page) pages of
    its own, in shuffled order; every later table entry names the one dead page (no position of it is ever live); three
    spare pages are named by nobody."""
    live = [(s + page - 1) // page for s in seqs]
    n_pages = sum(live) + 1 + 3
    ids = torch.randperm(n_pages, generator=g)
    dead = int(ids[sum(live)])
    table = torch.full((len(seqs), width), dead, dtype=torch.int32)
    unread = torch.ones(n_pages, page, dtype=torch.bool)
    at = 0
    for i, s in enumerate(seqs):
        mine = ids[at:at + live[i]]
        at += live[i]
        table[i, :live[i]] = mine.to(torch.int32)
        unread[mine] = torch.arange(live[i] * page).view(live[i], page) >= s
    assert unread[dead].all() and unread.sum() >= 4 * page
    return table, unread, dead


# ------------------------------------------------------------------------------------- flash_attn_with_kvcache, paged
def key_lengths(page):
    return [1, 31, 32, 33, page + 1, 2 * page - 1, 640]


def attn_paged_case(dtype, cache_dtype, seqs_q, seqs_k, Hq, Hk, D, page, causal, seed):
    """q, the clean and the poisoned K / V caches over one table, and the oracle of the live keys (the clean cache's own
    random values at the live positions are the logical inputs)"""
    g = torch.Generator().manual_seed(seed)
    b = len(seqs_k)
    q = torch.randn(sum(seqs_q), Hq, D, generator=g).to(dtype)
    cu_q = torch.tensor([0] + torch.cumsum(torch.tensor(seqs_q), 0).tolist(), dtype=torch.int32)
    table, unread, _ = paged_layout(seqs_k, page, (max(seqs_k) + page - 1) // page + 2, g)
    shape = (unread.shape[0], page, Hk, D)
    c = dict(q=q, cu_q=cu_q, table=table, scale=D ** -0.5, descale={})
    for name in ("k", "v"):
        x = torch.randn(shape, generator=g)
        if cache_dtype != dtype:  # an fp8 cache with one per-tensor descale, as test_fp8_kvcache builds it
            ds = x.abs().max().item() / (448.0 if cache_dtype == torch.float8_e4m3fn else 57344.0)
            c["descale"][name + "_descale"] = ds
            x = x / ds
        clean = x.to(cache_dtype)
        c[name + "_clean"], c[name + "_poisoned"] = clean, with_poison(clean, unread[:, :, None, None])
        audit(c[name + "_poisoned"], clean, unread[:, :, None, None])
        live = [oa.gather_paged(c[name + "_poisoned"], table[i], seqs_k[i]) for i in range(b)]
        assert all(torch.isfinite(x.float()).all() for x in live)
        c[name + "_live"] = [oa.dequant_fp8_cache(x, ds) for x in live] if cache_dtype != dtype else live
    c["ref"], c["ref_lse"] = oa.attention_ragged(q, c["k_live"], c["v_live"], cu_q, c["scale"], causal=causal)
    if cache_dtype == dtype:
        c["pt"] = torch.cat([pt_seq(q[cu_q[i]:cu_q[i + 1]], c["k_live"][i], c["v_live"][i], c["scale"], causal, (-1, -1), 0.0, None)
                             for i in range(b)])
    return c


def attn_paged_both(sglk, dev, c, seqs_q, seqs_k, causal, splits_list=(0,)):
    """both runs at every split count: (a) bits, (b) the rule of test_attention_gpu.run_paged / test_fp8_kvcache"""
    fixed = dict(cache_seqlens=torch.tensor(seqs_k, dtype=torch.int32, device=dev), page_table=c["table"].to(dev),
                 cu_seqlens_q=c["cu_q"].to(dev), max_seqlen_q=max(seqs_q), softmax_scale=c["scale"], causal=causal,
                 return_softmax_lse=True)
    for name, ds in c["descale"].items():
        fixed[name] = torch.tensor([ds], dtype=torch.float32, device=dev)
    q = c["q"].to(dev)
    caches = {kind: (c["k_" + kind].to(dev), c["v_" + kind].to(dev)) for kind in ("clean", "poisoned")}
    for splits in splits_list:
        res = {kind: sglk.flash_attn_with_kvcache(q, kc, vc, num_splits=splits, **fixed) for kind, (kc, vc) in caches.items()}
        out, lse = res["poisoned"][0].cpu(), res["poisoned"][1].cpu()
        what = f"splits={splits}"
        same_bits(out, res["clean"][0], what + " out")
        same_bits(lse, res["clean"][1], what + " lse")
        if "pt" in c:
            check(out, c["ref"], c["pt"], what)
        else:  # fp8 cache: the bounds of test_fp8_kvcache
            diff = (out.float() - c["ref"]).abs()
            assert diff.max().item() <= 2e-2 and diff.mean().item() <= 2e-3, (what, diff.max().item(), diff.mean().item())
        fin = torch.isfinite(c["ref_lse"])
        torch.testing.assert_close(lse[fin], c["ref_lse"][fin], rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize("page", [16, 64])
def test_attn_decode_kernel(sglk, dev, page):
    """sq = 1, d = 128: the independent-wave decode kernel (a 16-token page: a tile's two halves in two pages), one pass and split-KV"""
    seqs_k = key_lengths(page)
    seqs_q = [1] * len(seqs_k)
    c = attn_paged_case(torch.bfloat16, torch.bfloat16, seqs_q, seqs_k, 16, 4, 128, page, False, seed=page)
    attn_paged_both(sglk, dev, c, seqs_q, seqs_k, False, splits_list=(0, 1, 5))


@pytest.mark.parametrize("page", [8, 64])
def test_attn_prefill_kernel(sglk, dev, page):
    """200 causal queries, d = 128: the 128-row-block prefill kernel (8-token pages: the per-lane address path)"""
    seqs_k = key_lengths(page)
    seqs_q = [min(200, k) for k in seqs_k]
    c = attn_paged_case(torch.bfloat16, torch.bfloat16, seqs_q, seqs_k, 8, 2, 128, page, True, seed=page + 1)
    attn_paged_both(sglk, dev, c, seqs_q, seqs_k, True)


@pytest.mark.parametrize("D,sq,heads,dtype", [(80, 20, (6, 2), torch.float16), (512, 3, (8, 2), torch.bfloat16)])
def test_attn_general_kernel(sglk, dev, D, sq, heads, dtype):
    seqs_k = key_lengths(64)
    seqs_q = [min(sq, k) for k in seqs_k]
    c = attn_paged_case(dtype, dtype, seqs_q, seqs_k, heads[0], heads[1], D, 64, True, seed=D)
    attn_paged_both(sglk, dev, c, seqs_q, seqs_k, True)


@pytest.mark.parametrize("fp8_dtype", [torch.float8_e4m3fn, torch.float8_e5m2], ids=["e4m3", "e5m2"])
@pytest.mark.parametrize("page", [16, 64])
@pytest.mark.parametrize("sq", [1, 200])
def test_attn_fp8_kvcache(sglk, dev, sq, page, fp8_dtype):
    seqs_k = key_lengths(page)
    seqs_q = [min(sq, k) for k in seqs_k]
    c = attn_paged_case(torch.bfloat16, fp8_dtype, seqs_q, seqs_k, 8, 2, 128, page, sq > 1, seed=page + sq)
    attn_paged_both(sglk, dev, c, seqs_q, seqs_k, sq > 1)


# ----------------------------------------------------- flash_attn_with_kvcache, 4-D cache rows (no page table)
@pytest.mark.parametrize("use_batch_idx", [False, True])
@pytest.mark.parametrize("use_leftpad", [False, True])
@pytest.mark.parametrize("sq,D,heads", [(1, 128, (16, 4)), (40, 64, (8, 8))])
def test_attn_cache_rows(sglk, dev, use_batch_idx, use_leftpad, sq, D, heads):
    """built as test_kvcache_rows_batch_idx_leftpad: unread are the positions from cache_seqlens on, those in front of
    cache_leftpad, and (with cache_batch_idx) the two cache rows no sequence selects"""
    Hq, Hk = heads
    g = torch.Generator().manual_seed(sq + D + Hq)
    b, cache_len = 3, 448
    rows = 5 if use_batch_idx else b
    q = torch.randn(b, sq, Hq, D, generator=g).to(torch.bfloat16)
    batch_idx = torch.randperm(rows, generator=g)[:b].to(torch.int32) if use_batch_idx else None
    ends = torch.tensor([cache_len, 300, 225], dtype=torch.int32)  # the cache's end, inside a 32-token tile, one past a tile
    leftpad = torch.tensor([5, 37, 64], dtype=torch.int32) if use_leftpad else None
    unread = torch.ones(rows, cache_len, dtype=torch.bool)
    for i in range(b):
        row = int(batch_idx[i]) if use_batch_idx else i
        unread[row, (int(leftpad[i]) if use_leftpad else 0):int(ends[i])] = False
    unread = unread[:, :, None, None]
    caches = {}
    for name in ("k", "v"):
        clean = torch.randn(rows, cache_len, Hk, D, generator=g).to(torch.bfloat16)
        caches[name] = (clean, with_poison(clean, unread))
        audit(caches[name][1], clean, unread)
    d = lambda t: t.to(dev) if t is not None else None  # noqa: E731
    for causal in (False, True):
        res = [sglk.flash_attn_with_kvcache(d(q), d(caches["k"][kind]), d(caches["v"][kind]), cache_seqlens=d(ends),
                                            cache_batch_idx=d(batch_idx), cache_leftpad=d(leftpad), causal=causal,
                                            return_softmax_lse=True) for kind in (0, 1)]
        same_bits(res[1][0], res[0][0], f"causal={causal} out")
        same_bits(res[1][1], res[0][1], f"causal={causal} lse")
        out, lse = res[1][0].cpu().view(b, sq, Hq, D), res[1][1].cpu()
        for i in range(b):
            row = int(batch_idx[i]) if use_batch_idx else i
            lo, hi = (int(leftpad[i]) if use_leftpad else 0), int(ends[i])
            ki, vi = caches["k"][1][row, lo:hi], caches["v"][1][row, lo:hi]
            ref, ref_lse = oa.attention_seq(q[i], ki, vi, D ** -0.5, causal=causal)
            check(out[i], ref, pt_seq(q[i], ki, vi, D ** -0.5, causal, (-1, -1), 0.0, None), f"seq {i}")
            torch.testing.assert_close(lse[:, i * sq:(i + 1) * sq], ref_lse, rtol=1e-3, atol=1e-3)


# ------------------------------------------------------------------------------ flash_mla_decode / flash_mla_prefill
MLA_SEQS = [1, 17, 33, 100, 129]  # one key; one past a 16-token page; one past a tile; inside a tile; one past four tiles


def mla_caches(dtype, seqs, page, seed):
    """-> g, table (as wide as run_case makes it), dead page id, clean and poisoned latent cache [pages, page, 576]"""
    g = torch.Generator().manual_seed(seed)
    pack = 128 // page
    block_num = ((max(seqs) + page - 1) // page + pack - 1) // pack * pack
    table, unread, dead = paged_layout(seqs, page, block_num, g)
    clean = torch.randn(unread.shape[0], page, 576, generator=g).to(dtype)
    poisoned = with_poison(clean, unread[:, :, None])
    audit(poisoned, clean, unread[:, :, None])
    for i, s in enumerate(seqs):  # what the oracle reads is live
        assert torch.isfinite(poisoned[table[i].long()].reshape(-1, 576)[:s].float()).all()
    return g, table, dead, clean, poisoned


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("page", [16, 64])
@pytest.mark.parametrize("H", [16, 128])
def test_mla_decode(sglk, dev, H, page, dtype):
    """H = 16: the 16-head kernel, H = 128: the 128-row kernel; a 16-token page makes a 32-token tile span two pages. The
    last launch sits behind a table of 400k tokens (run_case's table_tokens): the launch is sized by the table's width."""
    g, table, dead, clean, poisoned = mla_caches(dtype, MLA_SEQS, page, seed=H + page)
    bs = len(MLA_SEQS)
    q = (torch.randn(bs, H, 576, generator=g) * 100.0).to(dtype)
    seq_lens = torch.tensor(MLA_SEQS, dtype=torch.int32)
    scale = (128 + 64) ** -0.5
    ref = omla.mla_decode(q, clean, scale, table, seq_lens)
    wide = torch.full((bs, (400_000 + 127) // 128 * (128 // page)), dead, dtype=torch.int32)
    wide[:, :table.shape[1]] = table
    qd = q.to(dev)
    q_nope, q_pe = qd[:, :, :512], qd[:, :, 512:].contiguous()
    caches = (clean.to(dev), poisoned.to(dev))
    atol, rtol = (1e-2, 1e-2) if dtype == torch.bfloat16 else (1e-3, 1e-3)  # test_mla_decode_gpu.run_case
    for tab, splits in ((table, -1), (table, 1), (table, 4), (wide, -1)):
        ws_size = sglk.flash_mla_get_workspace_size(tab.shape[1] * page, bs, H, page, num_kv_splits=splits)
        outs = [sglk.flash_mla_decode(q_nope, q_pe, cache, seq_lens.to(dev), tab.to(dev),
                                      torch.empty(ws_size, device=dev, dtype=torch.uint8), scale, splits).cpu() for cache in caches]
        what = f"splits={splits} table width {tab.shape[1]}"
        same_bits(outs[1], outs[0], what)
        torch.testing.assert_close(outs[1].float(), ref.float(), atol=atol, rtol=rtol, msg=lambda m: what + ": " + m)


@pytest.mark.parametrize("page", [16, 64])
@pytest.mark.parametrize("H", [16, 128])
def test_mla_prefill(sglk, dev, H, page):
    """arguments as test_mla_prefill_gpu.run_case builds them; causal, the new tokens are each sequence's last ones"""
    dtype = [torch.bfloat16, torch.float16][(page // 16 + H // 16) % 2]
    sqs, sks = [1, 17, 20, 33, 50], MLA_SEQS
    g, table, _, clean, poisoned = mla_caches(dtype, sks, page, seed=H + page + 1)
    cu = torch.tensor([0] + torch.cumsum(torch.tensor(sqs), 0).tolist(), dtype=torch.int32)
    sk = torch.tensor(sks, dtype=torch.int32)
    qn = torch.randn(sum(sqs), H, 512, generator=g).to(dtype)
    qp = torch.randn(sum(sqs), H, 64, generator=g).to(dtype)
    scale = (128 + 64) ** -0.5
    ref = omla.mla_prefill(qn, qp, clean, scale, table, cu, sk, causal=True)
    ws = torch.empty(sglk.flash_mla_prefill_get_workspace_size(table.shape[1] * page, len(sqs)), device=dev, dtype=torch.uint8)
    outs = [sglk.flash_mla_prefill(qn.to(dev), qp.to(dev), cache.to(dev), cu.to(dev), sk.to(dev), max(sqs), table.to(dev), ws,
                                   scale, causal=True, num_kv_splits=1).cpu() for cache in (clean, poisoned)]
    same_bits(outs[1], outs[0], "prefill")
    atol, rtol = (1e-2, 1e-2) if dtype == torch.bfloat16 else (1e-3, 1e-3)
    torch.testing.assert_close(outs[1].float(), ref.float(), atol=atol, rtol=rtol)


# ------------------------------------------------------------------------------------------------------- MQA logits
@pytest.mark.parametrize("H", [4, 64])
@pytest.mark.parametrize("page_size", [1, 4, 64])
@pytest.mark.parametrize("block", [False, True], ids=["row", "block"])
def test_mqa_paged(sglk, dev, block, page_size, H):
    """every byte of the cache that is no live key or live scale - positions from seq_len on in both layouts, the table's
    padding pages, the spare pages - holds 0x7F as a key byte and NaN as a scale"""
    seq_lens, max_seq_len = [0, 1, 2 * page_size + 3, 129], 199
    q, cache, w, table = make_paged(4, H, page_size, seq_lens, max_seq_len, block, seed=page_size + H)
    ko, so = slots(table, page_size, max_seq_len, block)
    live = torch.arange(max_seq_len)[None] < torch.tensor(seq_lens)[:, None]
    flat = cache.view(-1)
    keep = torch.zeros(flat.numel(), dtype=torch.bool)
    keep[(ko[live][:, None] + torch.arange(MQA_D)).view(-1)] = True
    keep[(so[live][:, None] + torch.arange(4)).view(-1)] = True
    off = torch.arange(flat.numel()) % (page_size * (MQA_D + 4))  # inside the page: which bytes hold scales, and which of the four
    sb = off - page_size * MQA_D if block else off % (MQA_D + 4) - MQA_D
    nan4 = torch.tensor([float("nan")]).view(torch.uint8)
    pat = torch.where(sb >= 0, nan4[sb.clamp(min=0) % 4], torch.full_like(flat, 0x7F))
    poisoned = torch.where(keep, flat, pat).view(cache.shape)
    # audit: the live keys and scales are those of the clean cache and finite, every other position within max_seq_len
    # decodes to NaN keys and a NaN scale, and so does every spare page
    pf = poisoned.view(-1)
    assert (~keep).sum() >= 3 * page_size * (MQA_D + 4) and torch.equal(pf[keep], flat[keep])
    keys = pf[ko[:, :, None] + torch.arange(MQA_D)].view(FP8).float()
    scales = pf[so[:, :, None] + torch.arange(4)].view(torch.float32).squeeze(-1)
    assert torch.isfinite(keys[live]).all() and torch.isfinite(scales[live]).all()
    assert torch.isnan(keys[~live]).all() and torch.isnan(scales[~live]).all() and (~live).sum() > 0
    spare = torch.ones(cache.shape[0], dtype=torch.bool)
    spare[table.view(-1).long()] = False
    assert spare.sum() == 3 and not keep.view(cache.shape[0], -1)[spare].any()

    ref, A, mask = paged_reference(q, cache, w, table, seq_lens, max_seq_len, block)  # on the clean cache
    assert torch.isfinite(ref).all()
    want = torch.where(mask, ref, torch.zeros_like(ref))
    fn = sglk.fp8_paged_mqa_logits_triton if block else sglk.fp8_paged_mqa_logits
    sl = torch.tensor(seq_lens, dtype=torch.int32, device=dev)
    outs = [fn(q.view(torch.uint8).to(dev).unsqueeze(1), c.to(dev), w.to(dev), sl, table.to(dev), None, max_seq_len).cpu()
            for c in (cache, poisoned)]
    same_bits(outs[1], outs[0], "paged logits")
    mqa_check(outs[1], want, A, mask)


def test_mqa_ragged(sglk, dev):
    """the windows() staircase with the last query's end clamped to 240: keys 240 .. 256 lie in no query's window"""
    Nq, Nk, H = 17, 257, 64
    q, k, k_scale, w = make_case(Nq, Nk, H, seed=Nq + Nk + H)
    ks, ke = windows(Nq, Nk)
    ke[-1] = 240
    j = torch.arange(Nk)[None]
    unread = ~((j >= ks[:, None]) & (j < ke[:, None])).any(0)
    assert torch.equal(unread.nonzero().flatten(), torch.arange(240, Nk))
    k_p = with_poison(k, unread[:, None])
    s_p = with_poison(k_scale, unread)
    s_p[unread] = float("nan")  # (scales: NaN only)
    audit(k_p, k, unread[:, None])
    audit(s_p, k_scale, unread)
    ref, A, mask = reference(q, k, k_scale, w, ks, ke)  # clean inputs
    want = torch.where(mask, ref, torch.zeros_like(ref))
    outs = [sglk.fp8_mqa_logits(q.to(dev), (kk.to(dev), ss.to(dev)), w.to(dev), ks.to(dev), ke.to(dev)).cpu()
            for kk, ss in ((k, k_scale), (k_p, s_p))]
    same_bits(outs[1], outs[0], "ragged logits")
    mqa_check(outs[1], want, A, mask)


# ------------------------------------------------------------------------------------------------------------ top-k
def test_topk_windows(sglk, dev):
    """test_misaligned_windows' layout (row stride > width, unaligned starts, two rows ending at the last column) and a row of
    len <= topk: +Inf / NaN in every column outside [row_start, row_start + len), the stride padding included"""
    g = torch.Generator().manual_seed(3)
    width, pad = 20001 + 7, 13
    starts, lengths = [7, 1, 2, width - 4099, 11], [20001, 4099, 20001, 4099, 1000]
    B = len(starts)
    clean = torch.randn(B, width + pad, generator=g)
    col = torch.arange(width + pad)[None]
    unread = (col < torch.tensor(starts)[:, None]) | (col >= (torch.tensor(starts) + torch.tensor(lengths))[:, None])
    assert unread[:, width:].all()
    poisoned = with_poison(clean, unread)
    audit(poisoned, clean, unread)
    assert torch.isinf(poisoned[unread]).any() and torch.isnan(poisoned[unread]).any()
    st, ln = i32(starts, dev), i32(lengths, dev)
    off = torch.randint(0, 10 ** 6, (B,), generator=g)
    cu = [0, 2, B]
    table = torch.stack([torch.randperm(width, generator=g) for _ in range(len(cu) - 1)])
    seq = torch.bucketize(torch.arange(B), torch.tensor(cu), right=True) - 1
    res = []
    for base in (clean, poisoned):
        score = base.to(dev)[:, :width]
        assert score.stride(0) > score.shape[1]
        res.append((sglk.fast_topk_v2(score, ln, K, st),
                    sglk.fast_topk_transform_ragged_fused(score, ln, i32(off, dev), K, st),
                    sglk.fast_topk_transform_fused(score, ln, i32(table, dev), i32(cu, dev), K, st)))
    for a, b_, what in zip(res[1], res[0], ("fast_topk_v2", "ragged_fused", "fused")):
        same_bits(a, b_, what)
    raw_p, ragged_p, fused_p = res[1]
    check_rows(clean[:, :width], raw_p, lengths, starts)
    r = raw_p.cpu().long()
    rows_equal(ragged_p, torch.where(r >= 0, r + off[:, None], -1))
    rows_equal(fused_p, torch.where(r >= 0, table[seq[:, None], r.clamp(min=0)], -1))
    assert torch.equal(fused_p[4].cpu().long(), torch.where(r[4] >= 0, table[1, r[4].clamp(min=0)], -1))  # len <= topk: slot by slot


@pytest.mark.parametrize("topk", [512, 2048])
def test_topk_transform_512_tail(sglk, dev, topk):
    g = torch.Generator().manual_seed(5)
    B, L, page_size = 3, 5120, 64
    lengths = [L - 1, 2500, min(topk, 700)]
    clean = torch.randn(B, L, generator=g)
    unread = torch.arange(L)[None] >= torch.tensor(lengths)[:, None]
    poisoned = with_poison(clean, unread)
    audit(poisoned, clean, unread)
    pages = torch.randperm(B * L // page_size, generator=g).view(B, L // page_size)
    res = []
    for base in (clean, poisoned):
        out = torch.empty(B, topk, dtype=torch.int32, device=dev)
        raw_idx = torch.empty_like(out)
        sglk.topk_transform_512(base.to(dev), i32(lengths, dev).view(B, 1), i32(pages, dev), out, page_size, raw_idx)
        res.append((out, raw_idx))
    same_bits(res[1][0], res[0][0], "page indices")
    same_bits(res[1][1], res[0][1], "raw indices")
    check_rows(clean, res[1][1], lengths, topk=topk)
    p = res[1][1].cpu().long()
    want = pages[torch.arange(B)[:, None], p.clamp(min=0) // page_size] * page_size + p.clamp(min=0) % page_size
    rows_equal(res[1][0], torch.where(p >= 0, want, -1))
