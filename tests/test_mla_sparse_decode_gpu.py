"""flash_mla_with_kvcache (sparse MLA decode over the packed fp8 cache) against a float64 CPU reference that unpacks the
cache bytes and follows the definition. Tolerances are the project's sparse-prefill bounds (dequantisation is exact, so the
error is that of the bf16 kernel): out atol = rtol = 1e-2 against the float64 result rounded to bf16, lse atol = rtol =
1e-3; +-inf entries compare equal."""
import ctypes
import functools
import os

import pytest
import torch

B = 3
# name -> (page_size, pages, extra_topk, extra pages, extra page size); "long" crosses 2048 slots and runs split
CONFIGS = {"none": (64, 3, 0, 0, 0), "small": (256, 2, 70, 40, 2), "long": (64, 3, 2100, 5, 64)}


def page_bytes(page_size):
    return 576 * page_size + -(-8 * page_size // 576) * 576


@functools.lru_cache(maxsize=None)
def build_cache(pages, page_size, seed):
    """uint8 [pages, page_bytes]: rows ~ randn quantised with a per-tile exponent byte in 124..130, rope randn in bf16"""
    g = torch.Generator().manual_seed(seed)
    ntok = pages * page_size
    exps = torch.randint(124, 131, (ntok, 7), generator=g)
    rows = torch.randn(ntok, 7, 64, generator=g) / torch.pow(2.0, exps.float() - 127)[..., None]
    rope = torch.randn(ntok, 64, generator=g).to(torch.bfloat16)
    data = torch.cat([rows.to(torch.float8_e4m3fn).view(ntok, 448).view(torch.uint8), rope.view(torch.uint8)], 1)
    scales = torch.zeros(ntok, 8, dtype=torch.uint8)
    scales[:, :7] = exps.to(torch.uint8)
    buf = torch.zeros(pages, page_bytes(page_size), dtype=torch.uint8)
    buf[:, :576 * page_size] = data.view(pages, -1)
    buf[:, 576 * page_size:584 * page_size] = scales.view(pages, -1)
    return buf


def unpack(buf, page_size):
    """float64 [tokens, 512]: e4m3 * 2^(scale byte - 127), then the rope"""
    ntok = buf.shape[0] * page_size
    data = buf[:, :576 * page_size].reshape(ntok, 576)
    scale = 2.0 ** (buf[:, 576 * page_size:584 * page_size].reshape(ntok, 8)[:, :7].double() - 127)
    nope = data[:, :448].contiguous().view(torch.float8_e4m3fn).float().double().view(ntok, 7, 64) * scale[..., None]
    return torch.cat([nope.view(ntok, 448), data[:, 448:].contiguous().view(torch.bfloat16).double()], 1)


def reference(q, lists, sm_scale, sink):
    """lists: (rows [tokens, 512] float64, indices [B, s_q, k], length [B] or None) per cache"""
    rows, valid = [], []
    for kv, idx, length in lists:
        idx = idx.long()
        ok = (idx >= 0) & (idx < kv.shape[0])
        if length is not None:
            ok &= torch.arange(idx.shape[2])[None, None, :] < length.long()[:, None, None]
        r = kv[idx.clamp(0, kv.shape[0] - 1)]
        r[~ok] = 0  # an invalid slot contributes nothing, whatever its token holds
        rows.append(r)
        valid.append(ok)
    rows, valid = torch.cat(rows, 2), torch.cat(valid, 2)
    P = sm_scale * torch.einsum("bshd,bskd->bshk", q.double(), rows)
    P = P.masked_fill(~valid[:, :, None, :], float("-inf"))
    lse = torch.logsumexp(P, dim=-1)
    lse_o = lse if sink is None else torch.logaddexp(lse, sink.double()[None, None, :])
    lonely = lse == float("-inf")
    w = torch.exp(P - lse_o.masked_fill(lonely, float("inf"))[..., None])
    out = torch.einsum("bshk,bskd->bshd", w, rows)
    return out.to(torch.bfloat16), lse.masked_fill(lonely, float("inf")).permute(0, 2, 1).float()


def make_indices(g, s_q, topk, ntok):
    idx = torch.randint(0, ntok, (B, s_q, topk), generator=g, dtype=torch.int32)
    hit = torch.rand(B, s_q, topk, generator=g) < 0.2  # invalid entries scattered through the list
    idx[hit] = torch.tensor([-1, ntok, ntok + 100], dtype=torch.int32)[torch.randint(0, 3, (int(hit.sum()),), generator=g)]
    return idx


def make_case(cfg, h_q, topk, s_q=1, lengths=False, seed=0):
    page_size, pages, extra_topk, extra_pages, extra_page_size = CONFIGS[cfg]
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, s_q, h_q, 512, generator=g).to(torch.bfloat16)
    idx = make_indices(g, s_q, topk, pages * page_size)
    idx[1, 0, :32] = -1  # a token whose first 32 main slots are all invalid
    caches = [(build_cache(pages, page_size, 11), page_size, idx,
               torch.tensor([topk, max(1, topk // 2), 1], dtype=torch.int32) if lengths else None)]
    if extra_topk:
        caches.append((build_cache(extra_pages, extra_page_size, 12), extra_page_size,
                       make_indices(g, s_q, extra_topk, extra_pages * extra_page_size),
                       torch.tensor([extra_topk, 40, extra_topk // 2], dtype=torch.int32) if lengths else None))
    return q, caches


def run(sglk, dev, q, caches, sm_scale, sink):
    def on_dev(buf, page_size):
        return buf.to(dev).view(torch.float8_e4m3fn).as_strided((buf.shape[0], page_size, 1, 584), (buf.shape[1], 576, 576, 1))

    on = lambda t: None if t is None else t.to(dev)
    extra = caches[1] if len(caches) > 1 else (None, 0, None, None)
    out, lse = sglk.flash_mla_with_kvcache(
        on(q), on_dev(*caches[0][:2]), softmax_scale=sm_scale, is_fp8_kvcache=True, indices=on(caches[0][2]),
        attn_sink=on(sink), extra_k_cache=None if extra[0] is None else on_dev(*extra[:2]),
        extra_indices_in_kvcache=on(extra[2]), topk_length=on(caches[0][3]), extra_topk_length=on(extra[3]))
    return out.cpu(), lse.cpu()


def check(got, q, caches, sm_scale, sink):
    r_out, r_lse = reference(q, [(unpack(buf, ps), idx, ln) for buf, ps, idx, ln in caches], sm_scale, sink)
    assert got[0].dtype == torch.bfloat16 and got[1].dtype == torch.float32
    torch.testing.assert_close(got[1], r_lse, atol=1e-3, rtol=1e-3)
    torch.testing.assert_close(got[0].float(), r_out.float(), atol=1e-2, rtol=1e-2)


@pytest.mark.gpu
@pytest.mark.parametrize("extras", ["plain", "sink", "length", "sink+length"])
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("topk", [6, 33, 160])
@pytest.mark.parametrize("h_q", [8, 24, 64, 128])
def test_decode_parity(sglk, dev, h_q, topk, cfg, extras):
    s_q = 2 if (h_q, topk, cfg) == (24, 33, "small") else 1
    q, caches = make_case(cfg, h_q, topk, s_q, "length" in extras, seed=h_q + topk)
    sink = None
    if "sink" in extras:
        sink = torch.randn(h_q, generator=torch.Generator().manual_seed(7))
        sink[1], sink[h_q - 2] = float("inf"), float("-inf")
    check(run(sglk, dev, q, caches, 0.09, sink), q, caches, 0.09, sink)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,h_q", [("small", 24), ("long", 128)])
def test_decode_lonely_query(sglk, dev, cfg, h_q):
    q, caches = make_case(cfg, h_q, 70, seed=3)
    for _, _, idx, _ in caches:
        idx[2] = -1 - idx[2].abs()
    sink = torch.zeros(h_q)
    got = run(sglk, dev, q, caches, 0.07, sink)
    assert (got[0][2] == 0).all() and (got[1][2] == float("inf")).all()
    check(got, q, caches, 0.07, sink)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,h_q", [("small", 24), ("long", 128)])
def test_decode_poisoned_cache(sglk, dev, cfg, h_q):
    """every cache token that no valid slot names holds fp8 NaN bytes (data and rope) and scale bytes 0xFF"""
    q, caches = make_case(cfg, h_q, 70, lengths=True, seed=5)
    poisoned, tokens = [], 0
    for buf, ps, idx, length in caches:
        ntok = buf.shape[0] * ps
        live = (torch.arange(idx.shape[2])[None, None, :] < length[:, None, None]) & (idx >= 0) & (idx < ntok)
        unused = torch.ones(ntok, dtype=torch.bool)
        unused[idx[live].long()] = False
        tokens += int(unused.sum())
        bad = buf.clone()
        bad[:, :576 * ps].unflatten(1, (ps, 576))[unused.view(-1, ps)] = 0x7F
        bad[:, 576 * ps:584 * ps].unflatten(1, (ps, 8))[unused.view(-1, ps)] = 0xFF
        poisoned.append((bad, ps, idx, length))
    assert tokens > 50
    clean = run(sglk, dev, q, caches, 0.07, None)
    got = run(sglk, dev, q, poisoned, 0.07, None)
    for a, b in zip(got, clean):
        assert torch.isfinite(a).all() and torch.equal(a, b)


def test_auto_splits():
    """the parity cases of the long configuration (3 tokens, >= 2106 slots) run split, a full batch does not"""
    lib = ctypes.CDLL(os.path.join(os.path.dirname(__file__), "..", "sgl-kernel-xpu_amd", "python", "sgl_kernel", "libsglk.so"))
    f = lib.sglk_mla_sparse_decode_auto_splits
    f.restype, f.argtypes = ctypes.c_int64, [ctypes.c_int64] * 3
    assert f(1, 1, 2260) > 1 and f(3, 1, 2106) > 1
    assert f(512, 1, 640) == 1


def test_rejected_arguments(sglk):
    q = torch.zeros(1, 1, 8, 512, dtype=torch.bfloat16)
    cache = torch.zeros(1, 64, 1, 584).to(torch.float8_e4m3fn)
    idx = torch.zeros(1, 1, 4, dtype=torch.int32)
    ok = dict(is_fp8_kvcache=True, indices=idx)
    for bad, err in ((dict(tile_scheduler_metadata=idx), AssertionError), (dict(num_splits=idx), AssertionError),
                     (dict(causal=True), AssertionError), (dict(block_table=idx), NotImplementedError),
                     (dict(is_fp8_kvcache=False), AssertionError), (dict(extra_k_cache=cache), AssertionError),
                     (dict(extra_indices_in_kvcache=idx), AssertionError)):
        with pytest.raises(err):
            sglk.flash_mla_with_kvcache(q, cache, **{**ok, **bad})
