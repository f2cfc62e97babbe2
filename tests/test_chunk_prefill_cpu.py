"""Chunked prefill into the paged KV cache, off the GPU: ``generate_continuous(prefill_chunk=32)`` against the unchunked
run on the float32 model, ``write_rows`` in pieces against ``load_row``, and the CPU path of ``chunk_attention``."""
import pytest
import torch

from batch_decode_common import make_model
from scaling_amd.core.nn.attention.attention import KVCache, PagedDecodeState, PagedKVCache, PagedKVCacheFP8
from scaling_amd.ops import attention, quant

FP8 = "fp8_e4m3"
LENGTHS = [5, 32, 33, 70]  # one short chunk, exactly one chunk, one token into the second, three chunks


@pytest.fixture(scope="module")
def model():
    return make_model("cpu", "float32")


@pytest.mark.parametrize("kv_cache", [None, FP8])
def test_chunked_generation_returns_the_unchunked_tokens(model, kv_cache):
    """Greedy tokens.  The two runs differ by float32 summation order (chunked against one-shot matmuls) and, with the
    FP8 cache, by the prompt's later chunks reading its keys as e4m3 codes; seed 0's prompts keep every argmax of the
    unchunked run clear of both."""
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(1, 256, (n,), generator=g).tolist() for n in LENGTHS]
    kw = dict(input_tokens=prompts, max_batch=2, page_size=32, stop_tokens=[], kv_cache=kv_cache)
    ref = model.generate_continuous(6, **kw)
    got = model.generate_continuous(6, prefill_chunk=32, **kw)
    assert [o.completion_tokens for o in got] == [o.completion_tokens for o in ref]
    assert all(torch.isfinite(o.completion_logits).all() for o in got)
    with pytest.raises(ValueError, match="multiple of 32"):
        model.generate_continuous(6, prefill_chunk=48, **kw)


@pytest.mark.parametrize("fp8", [False, True])
def test_write_rows_in_pieces_equals_load_row(fp8):
    torch.manual_seed(1)
    nkv, hd, page, n = 2, 16, 32, 96
    pages = [5, 2, 7]
    st = PagedDecodeState(2, 4, page, 9, torch.device("cpu"))
    cls, dtype = (PagedKVCacheFP8, torch.bfloat16) if fp8 else (PagedKVCache, torch.float32)
    k, v = torch.randn(2, n, nkv, hd).to(dtype)
    whole, pieces = cls.empty(nkv, hd, dtype, st), cls.empty(nkv, hd, dtype, st)
    whole.load_row(0, KVCache(k, v, n), pages)
    at = 0
    for m in (1, 31, 64):
        pieces.write_rows(pages, at, k[at : at + m], v[at : at + m])
        at += m
    names = ("k", "v", "k_scale", "v_scale") if fp8 else ("k", "v")
    for name in names:
        assert torch.equal(getattr(pieces, name), getattr(whole, name)), name
    st.check()


@pytest.mark.parametrize("fp8", [False, True])
def test_cpu_chunk_attention_is_the_reference_on_the_gathered_keys(fp8):
    torch.manual_seed(2)
    Hk, grp, D, page = 2, 2, 16, 32
    lq, lk = [40, 3], [71, 35]
    table = torch.tensor([[4, 1, 6], [3, 5, -1]], dtype=torch.int32)
    k, v = torch.randn(2, 7 * page, Hk, D)
    q = torch.randn(sum(lq), Hk * grp, D)
    cu_q = torch.tensor([0, 40, 43], dtype=torch.int32)
    k_range = torch.tensor([[0, n] for n in lk], dtype=torch.int32)
    scales = None
    if fp8:
        (k, ks), (v, vs) = quant.quantize_kv_rows(k.bfloat16()), quant.quantize_kv_rows(v.bfloat16())
        scales = (ks, vs)
    got = attention.chunk_attention(q, k, v, cu_q, k_range, 40, 71, 0.25, window=20, local_heads=3, kv_scales=scales,
                                    block_table=table, page_size=page)
    rows, ranges = attention.gather_pages(table, page, lk)
    if fp8:
        k, v = quant.dequantize_kv_rows(k, ks, q.dtype), quant.dequantize_kv_rows(v, vs, q.dtype)
    ref = attention.attention_reference(q, k[rows], v[rows], cu_q, None, 0.25, True, 20, local_heads=3, key_ranges=ranges)
    assert torch.equal(got, ref)
