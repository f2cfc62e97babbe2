"""Batched generation on the CPU path (``generate_batch``, eager): key ranges in ``attention_reference``, batched
versus single-sequence generation on a float32 model, per-row stop tokens and the argument errors."""
import pytest
import torch

from batch_decode_common import MAX_TOKENS, PROMPTS, make_model
from scaling_amd.ops.attention import attention_reference, flash_attention

RANGES = [(0, 1), (100, 33), (200, 64), (300, 0)]


@pytest.fixture(scope="module")
def model():
    return make_model("cpu", "float32")


@pytest.fixture(scope="module")
def singles(model):
    """generate(use_cache=True) of the first four prompts, computed once."""
    return [model.generate(MAX_TOKENS, input_tokens=p, stop_tokens=[], use_cache=True) for p in PROMPTS[:4]]


@pytest.mark.parametrize("lq", [1, 2])
def test_key_ranges_reference_equals_compacted(lq):
    g = torch.Generator().manual_seed(0)
    hq, hk, d = 4, 2, 64
    nseg = len(RANGES)
    k = torch.full((400, hk, d), float("nan"))
    v = torch.full((400, hk, d), float("nan"))
    for s0, n in RANGES:
        k[s0 : s0 + n] = torch.randn(n, hk, d, generator=g)
        v[s0 : s0 + n] = torch.randn(n, hk, d, generator=g)
    q = torch.randn(nseg * lq, hq, d, generator=g)
    cu_q = torch.arange(nseg + 1, dtype=torch.int32) * lq
    kc = torch.cat([k[s0 : s0 + n] for s0, n in RANGES])
    vc = torch.cat([v[s0 : s0 + n] for s0, n in RANGES])
    cu_k = torch.tensor([0] + [n for _, n in RANGES], dtype=torch.int32).cumsum(0).to(torch.int32)
    kr = torch.tensor(RANGES, dtype=torch.int32)
    ref = attention_reference(q, kc, vc, cu_q, cu_k, 0.125, True)
    out = attention_reference(q, k, v, cu_q, None, 0.125, True, key_ranges=kr)
    assert torch.isfinite(out).all()
    assert torch.equal(out, ref)
    # the public entry point takes the same argument (CPU tensors: the reference)
    with torch.no_grad():
        pub = flash_attention(q, k, v, cu_q, max_seqlen_q=lq, max_seqlen_k=100, softmax_scale=0.125, key_ranges=kr)
    assert torch.equal(pub, ref)


def test_prompts_have_a_clear_top_two_margin(singles):
    """The token comparison below is meaningful only if no step is a near tie (fp32 sum-order noise ~1e-6)."""
    for p, s in zip(PROMPTS, singles):
        assert len(s.completion_tokens) == MAX_TOKENS
        top = s.completion_logits.topk(2, dim=-1).values
        assert float((top[:, 0] - top[:, 1]).min()) >= 1e-3, (len(p), float((top[:, 0] - top[:, 1]).min()))


@pytest.mark.parametrize("B", [1, 2, 4])
def test_batched_equals_single_on_cpu(model, singles, B):
    outs = model.generate_batch(MAX_TOKENS, input_tokens=PROMPTS[:B], stop_tokens=[])
    assert len(outs) == B
    for o, s in zip(outs, singles):
        assert o.completion_tokens == s.completion_tokens
        assert o.completion_logits.shape == s.completion_logits.shape == (MAX_TOKENS, 256)
        # fp32 sum-order noise on O(1) logits is ~1e-6; the bound leaves two orders
        torch.testing.assert_close(o.completion_logits, s.completion_logits, rtol=0, atol=1e-4)


def test_per_row_stop_tokens(model, singles):
    # one stop token taken from each row's own text, at a different step per row
    stops = [s.completion_tokens[5 + 6 * b] for b, s in enumerate(singles)]
    want = [model.generate(MAX_TOKENS, input_tokens=p, stop_tokens=stops, use_cache=True) for p in PROMPTS[:4]]
    lengths = [len(w.completion_tokens) for w in want]
    assert len(set(lengths)) > 1 and min(lengths) < MAX_TOKENS, lengths  # the rows stop at different steps
    outs = model.generate_batch(MAX_TOKENS, input_tokens=PROMPTS[:4], stop_tokens=stops)
    for o, w in zip(outs, want):
        assert o.completion_tokens == w.completion_tokens
        assert o.completion_tokens[-1] in stops or len(o.completion_tokens) == MAX_TOKENS
        assert not any(t in stops for t in o.completion_tokens[:-1])
        assert o.completion_logits.shape[0] == len(o.completion_tokens)
        torch.testing.assert_close(o.completion_logits, w.completion_logits, rtol=0, atol=1e-4)


def test_argument_errors(model):
    with pytest.raises(ValueError, match="no prompts"):
        model.generate_batch(4, input_tokens=[], stop_tokens=[])
    with pytest.raises(ValueError, match="empty prompt"):
        model.generate_batch(4, input_tokens=[[1, 2], []], stop_tokens=[])
    with pytest.raises(ValueError, match="use_cuda_graph supports at most 4"):
        model.generate_batch(4, input_tokens=[[1, 2]] * 5, stop_tokens=[], use_cuda_graph=True)
