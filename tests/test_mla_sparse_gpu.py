"""GPU parity: flash_mla_sparse_fwd against a float64 CPU reference that follows the definition (reference
tests/test_flash_mla_sparse_fwd.py:26-68). Tolerances are the reference test's (:134-136): out atol = rtol = 1e-2
against the float64 result rounded to bf16, max_logits and lse atol = rtol = 1e-3; +-inf entries compare equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu

S_Q, S_KV = 5, 300


def reference(q, kv, indices, sm_scale, sink=None, topk_length=None):
    s_kv, topk = kv.shape[0], indices.shape[2]
    idx = indices[:, 0].long()
    valid = (idx >= 0) & (idx < s_kv)
    if topk_length is not None:
        valid &= torch.arange(topk)[None, :] < topk_length[:, None].long()
    rows = kv[:, 0].double()[idx.clamp(0, s_kv - 1)]  # [s_q, topk, d_qk]
    rows[~valid] = 0  # an invalid slot contributes nothing, whatever its row holds
    P = sm_scale * torch.einsum("thd,tkd->thk", q.double(), rows)
    P = P.masked_fill(~valid[:, None, :], float("-inf"))
    max_logits, lse = P.max(dim=-1).values, torch.logsumexp(P, dim=-1)
    lse_o = lse if sink is None else torch.logaddexp(lse, sink.double()[None, :])
    lonely = lse == float("-inf")
    w = torch.exp(P - lse_o.masked_fill(lonely, float("inf"))[..., None])
    out = torch.einsum("thk,tkd->thd", w, rows[..., :512])
    return out.to(torch.bfloat16), max_logits.float(), lse.masked_fill(lonely, float("inf")).float()


def make_case(d_qk, h_q, topk, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(S_Q, h_q, d_qk, generator=g).to(torch.bfloat16)
    kv = torch.randn(S_KV, 1, d_qk, generator=g).to(torch.bfloat16)
    indices = torch.randint(0, S_KV, (S_Q, 1, topk), generator=g, dtype=torch.int32)
    bad = torch.tensor([-1, S_KV, S_KV + 100], dtype=torch.int32)
    hit = torch.rand(S_Q, 1, topk, generator=g) < 0.2  # invalid entries scattered through the lists
    indices[hit] = bad[torch.randint(0, 3, (int(hit.sum()),), generator=g)]
    indices[1, 0, :32] = -1  # a token whose first whole tile is invalid
    return q, kv, indices


def run(sglk, dev, q, kv, indices, sm_scale, sink, topk_length):
    on = lambda t: None if t is None else t.to(dev)
    res = sglk.flash_mla_sparse_fwd(on(q), on(kv), on(indices), sm_scale, 512, on(sink), on(topk_length))
    return [t.cpu() for t in res]


def check(got, ref):
    out, max_logits, lse = got
    r_out, r_max, r_lse = ref
    assert out.dtype == torch.bfloat16 and max_logits.dtype == lse.dtype == torch.float32
    torch.testing.assert_close(max_logits, r_max, atol=1e-3, rtol=1e-3)
    torch.testing.assert_close(lse, r_lse, atol=1e-3, rtol=1e-3)
    torch.testing.assert_close(out.float(), r_out.float(), atol=1e-2, rtol=1e-2)


@pytest.mark.parametrize("extras", ["plain", "sink", "length", "sink+length"])
@pytest.mark.parametrize("topk", [6, 33, 160])
@pytest.mark.parametrize("h_q", [8, 24, 64, 128])
@pytest.mark.parametrize("d_qk", [512, 576])
def test_sparse_parity(sglk, dev, d_qk, h_q, topk, extras):
    q, kv, indices = make_case(d_qk, h_q, topk, seed=h_q + topk)
    g = torch.Generator().manual_seed(7)
    sink = topk_length = None
    if "sink" in extras:
        sink = torch.randn(h_q, generator=g)
        sink[1], sink[h_q - 2] = float("inf"), float("-inf")
    if "length" in extras:
        topk_length = torch.randint(1, topk + 1, (S_Q,), generator=g, dtype=torch.int32)
    sm_scale = (128 if d_qk == 512 else 192) ** -0.5
    check(run(sglk, dev, q, kv, indices, sm_scale, sink, topk_length), reference(q, kv, indices, sm_scale, sink, topk_length))


@pytest.mark.parametrize("h_q", [24, 128])
def test_sparse_lonely_query(sglk, dev, h_q):
    q, kv, indices = make_case(576, h_q, 70, seed=3)
    indices[2] = torch.tensor([-1, S_KV, S_KV + 100, -5] * 18)[:70]
    got = run(sglk, dev, q, kv, indices, 0.07, torch.zeros(h_q), None)
    assert (got[0][2] == 0).all() and (got[1][2] == float("-inf")).all() and (got[2][2] == float("inf")).all()
    check(got, reference(q, kv, indices, 0.07, torch.zeros(h_q)))


@pytest.mark.parametrize("h_q", [24, 128])
def test_sparse_poisoned_rows(sglk, dev, h_q):
    """every kv row that no valid slot names is NaN: row 0, and the rows only slots at or past topk_length name"""
    q, kv, indices = make_case(576, h_q, 70, seed=5)
    indices[indices == 0] = 1
    topk_length = torch.tensor([70, 40, 33, 1, 64], dtype=torch.int32)
    live = torch.arange(70)[None, :] < topk_length[:, None]
    idx = indices[:, 0].long()
    used = idx[live & (idx >= 0) & (idx < S_KV)]
    poisoned = kv.clone()
    unused = torch.ones(S_KV, dtype=torch.bool)
    unused[used] = False
    assert unused[0] and unused.sum() > 1
    poisoned[unused] = float("nan")
    clean = run(sglk, dev, q, kv, indices, 0.07, None, topk_length)
    got = run(sglk, dev, q, poisoned, indices, 0.07, None, topk_length)
    for a, b in zip(got, clean):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b)
