"""Paged KV cache and continuous batching without a GPU (float32 CPU model): the page allocator, the cache classes'
unfused append across page boundaries, ``flash_attention(block_table=...)`` against the ``key_ranges`` reference on the
gathered rows, and ``generate_continuous`` against ``generate`` per prompt (bf16-free path and FP8 KV)."""
import pytest
import torch

import test_kv_fp8_cpu as fp8_ref
from batch_decode_common import PROMPTS, make_model
from scaling_amd.core.nn.attention.attention import (KVCache, PageAllocator, PagedDecodeState, PagedKVCache,
                                                     PagedKVCacheFP8)
from scaling_amd.ops import attention, quant
from scaling_amd.transformer.inference import ContinuousBatchDecoder, batch_decode

FP8 = "fp8_e4m3"
LIMITS = [5, 40, 12, 63, 20, 9]


# ---------------------------------------------------------------------------------------------- allocator
def test_allocator_allocates_frees_reuses_and_exhausts():
    al = PageAllocator(8, reserved=2)
    assert al.free_pages == 6 and al.in_use == 0
    a = al.alloc(3)
    b = al.alloc(2)
    assert len(set(a + b)) == 5 and all(2 <= p < 8 for p in a + b)  # never a parking page
    assert al.free_pages == 1 and al.in_use == 5 and al.peak_in_use == 5
    with pytest.raises(RuntimeError, match="8 pages"):
        al.alloc(2)
    assert al.free_pages == 1  # a refused request takes nothing
    al.free(a)
    assert al.free_pages == 4 and al.in_use == 2
    c = al.alloc(4)
    assert set(c) & set(a) == set(a) and not set(c) & set(b)  # freed pages are handed out again
    with pytest.raises(RuntimeError, match="out of pages"):
        al.alloc(1)
    with pytest.raises(AssertionError):
        al.free([0])  # a parking page was never allocated
    al.free(b + c)
    assert al.free_pages == 6 and al.peak_in_use == 6
    with pytest.raises(ValueError):
        PageAllocator(2, reserved=2)


def test_page_size_must_be_a_multiple_of_32():
    for bad in (0, 16, 48, -32):
        with pytest.raises(ValueError, match="multiple of 32"):
            PagedDecodeState(2, 2, bad, 8, torch.device("cpu"))
    PagedDecodeState(2, 2, 96, 8, torch.device("cpu"))


# ---------------------------------------------------------------------------------------------- cache classes
def _prefilled(n, nkv, hd, seed):
    g = torch.Generator().manual_seed(seed)
    k, v = torch.randn(n, nkv, hd, generator=g), torch.randn(n, nkv, hd, generator=g)
    return KVCache.start(k, v)


@pytest.mark.parametrize("fp8", [False, True])
def test_unfused_append_addresses_pages(fp8):
    page, nkv, hd = 32, 2, 16
    st = PagedDecodeState(3, 3, page, 3 + 6, torch.device("cpu"))
    cls = PagedKVCacheFP8 if fp8 else PagedKVCache
    cache = cls.empty(nkv, hd, torch.float32, st)
    # parked rows: position 0, one key, their own page
    assert st.pos.tolist() == [0, 0, 0] and st.k_range.tolist() == [[0, 1]] * 3 and st.live.tolist() == [0, 0, 0]
    assert st.block_table.tolist() == [[0, -1, -1], [1, -1, -1], [2, -1, -1]]
    pages = {0: [7, 4], 1: [5]}
    kvs = {0: _prefilled(31, nkv, hd, 1), 1: _prefilled(3, nkv, hd, 2)}
    for b in (0, 1):
        cache.load_row(b, kvs[b], pages[b])
        st.assign(b, pages[b], kvs[b].length)
    assert st.pos.tolist() == [31, 3, 0] and st.k_range[:, 1].tolist() == [32, 4, 1] and st.live.tolist() == [1, 1, 0]

    def dense(t):
        return quant.dequantize_kv_rows(t, cache.k_scale, torch.float32) if fp8 else t

    def rounded(x):
        return quant.dequantize_kv_rows(*quant.quantize_kv_rows(x.to(torch.bfloat16)), dtype=torch.float32) if fp8 else x

    assert torch.equal(dense(cache.k)[7 * page : 7 * page + 31], rounded(kvs[0].k[:31]))
    assert torch.equal(dense(cache.k)[5 * page : 5 * page + 3], rounded(kvs[1].k[:3]))
    g = torch.Generator().manual_seed(3)
    written = {}
    for step in range(3):  # row 0 writes 31 (end of page 7), 32 and 33 (page 4); the parked row its parking page
        k, v = torch.randn(3, nkv, hd, generator=g), torch.randn(3, nkv, hd, generator=g)
        kk, vv, kr = cache.append(k, v)
        assert kk is cache.k and kr is st.k_range
        for b, p in enumerate(st.pos.tolist()):
            row = st.block_table[b, p // page].item() * page + p % page
            written[row] = rounded(k)[b]
        st.advance()
    assert int(st.err.item()) == 0
    assert st.pos.tolist() == [34, 6, 0] and st.k_range[:, 1].tolist() == [35, 7, 1]
    assert sorted(written) == [2 * page, 4 * page, 4 * page + 1, 5 * page + 3, 5 * page + 4, 5 * page + 5, 7 * page + 31]
    for row, want in written.items():
        assert torch.equal(dense(cache.k)[row], want)
    # a row that runs past its pages, and one past the table: the error word, and nothing is written
    st.pos[1] = page  # row 1 owns one page
    st.pos[0] = 3 * page
    before = cache.k.clone()
    cache.append(k, v)
    assert int(st.err.item()) & 1
    changed = (cache.k != before).flatten(1).any(1).nonzero().flatten().tolist()
    assert changed in ([], [2 * page])  # only the parked row wrote (its own page)
    with pytest.raises(RuntimeError, match="outside its pages"):
        st.check()


def test_flash_attention_block_table_reference_equals_key_ranges_on_gathered_rows():
    page, Hk, D = 32, 2, 16
    lengths = [1, 33, 64, 70]
    tab = torch.tensor([[5, -1, -1], [2, 7, 2**30], [0, 3, -1], [6, 1, 4]], dtype=torch.int32)
    g = torch.Generator().manual_seed(4)
    k, v = torch.randn(8 * page, Hk, D, generator=g), torch.randn(8 * page, Hk, D, generator=g)
    q = torch.randn(4, 4, D, generator=g)
    cu = torch.arange(5, dtype=torch.int32)
    kr = torch.tensor([(0, n) for n in lengths], dtype=torch.int32)
    rows, ranges = attention.gather_pages(tab, page, lengths)
    assert ranges.tolist() == [[0, 1], [1, 33], [34, 64], [98, 70]]
    assert rows[1:34].tolist() == list(range(2 * page, 3 * page)) + [7 * page]
    ref = attention.flash_attention(q, k[rows], v[rows], cu, max_seqlen_q=1, max_seqlen_k=96, key_ranges=ranges)
    out = attention.flash_attention(q, k, v, cu, max_seqlen_q=1, max_seqlen_k=96, key_ranges=kr, block_table=tab,
                                    page_size=page)
    assert torch.equal(out, ref)
    kq, ks = quant.quantize_kv_rows(k.to(torch.bfloat16))
    vq, vs = quant.quantize_kv_rows(v.to(torch.bfloat16))
    ref8 = attention.flash_attention(q, kq[rows], vq[rows], cu, max_seqlen_q=1, max_seqlen_k=96, key_ranges=ranges,
                                     kv_scales=(ks[:, rows], vs[:, rows]))
    out8 = attention.flash_attention(q, kq, vq, cu, max_seqlen_q=1, max_seqlen_k=96, key_ranges=kr, kv_scales=(ks, vs),
                                     block_table=tab, page_size=page)
    assert torch.equal(out8, ref8)
    with pytest.raises(ValueError, match="multiple of 32"):
        attention.flash_attention(q, k, v, cu, max_seqlen_k=96, key_ranges=kr, block_table=tab, page_size=40)
    with pytest.raises(ValueError, match="key_ranges"):
        attention.flash_attention(q, k, v, cu, max_seqlen_k=96, block_table=tab, page_size=page)
    with pytest.raises(ValueError, match="int32"):
        attention.flash_attention(q, k, v, cu, max_seqlen_k=96, key_ranges=kr, block_table=tab.long(), page_size=page)


# ---------------------------------------------------------------------------------------------- generation
@pytest.fixture(scope="module")
def model():
    return make_model("cpu", "float32")


@pytest.fixture(scope="module")
def singles(model):
    return [model.generate(m, input_tokens=p, stop_tokens=[]) for p, m in zip(PROMPTS, LIMITS)]


def test_continuous_equals_generate_per_prompt(model, singles):
    stop = singles[3].completion_tokens[17]  # request 3 stops early; cut the references at the same token
    outs = model.generate_continuous(LIMITS, input_tokens=PROMPTS, max_batch=2, page_size=32, stop_tokens=[stop])
    assert len(outs) == len(PROMPTS)
    lengths = []
    for o, one in zip(outs, singles):
        want = one.completion_tokens
        cut = next((i + 1 for i, t in enumerate(want) if t == stop), len(want))
        assert o.completion_tokens == want[:cut]
        assert o.completion_logits.shape == (cut, 256)
        torch.testing.assert_close(o.completion_logits, one.completion_logits[:cut], rtol=0, atol=1e-4)
        lengths.append(cut)
    assert lengths[3] <= 18 and lengths[1] == 40


def test_paged_static_batch_equals_slab_batch(model):
    slab = model.generate_batch(63, input_tokens=PROMPTS[:4], stop_tokens=[])
    paged = model.generate_batch(63, input_tokens=PROMPTS[:4], stop_tokens=[], page_size=32)
    for s, p in zip(slab, paged):
        assert s.completion_tokens == p.completion_tokens
        assert torch.equal(s.completion_logits, p.completion_logits)


def test_continuous_with_fp8_cache_equals_the_dequantised_run(model, monkeypatch):
    outs = model.generate_continuous(LIMITS, input_tokens=PROMPTS, max_batch=2, page_size=32, stop_tokens=[], kv_cache=FP8)
    monkeypatch.setattr(batch_decode, "BatchStaticKVCache", fp8_ref._DequantisedBatchCache)
    for o, p, m in zip(outs, PROMPTS, LIMITS):
        oracle = model.generate_batch(m, input_tokens=[p], stop_tokens=[])[0]
        assert o.completion_tokens == oracle.completion_tokens
        torch.testing.assert_close(o.completion_logits, oracle.completion_logits, rtol=0, atol=1e-4)


def test_serve_recycles_rows_and_pages(model):
    dec = model.continuous_decoder(2, page_size=32, max_pages=3)
    assert isinstance(dec, ContinuousBatchDecoder) and dec.allocator.free_pages == 6
    done = dec.serve(list(zip(PROMPTS, LIMITS)), stop_tokens=[])
    assert [len(t) for t, _ in done] == LIMITS
    assert dec.allocator.free_pages == 6 and dec.allocator.in_use == 0  # everything but the parking pages
    assert dec.free_rows == [0, 1] and dec.state.live.tolist() == [0, 0]
    assert dec.allocator.peak_in_use <= 6 and dec.steps_run < sum(LIMITS)


def test_decoder_errors(model):
    with pytest.raises(ValueError, match="multiple of 32"):
        model.generate_continuous(4, input_tokens=PROMPTS[:2], max_batch=2, page_size=48, stop_tokens=[])
    with pytest.raises(ValueError, match="multiple of 32"):
        model.generate_batch(4, input_tokens=PROMPTS[:2], stop_tokens=[], page_size=20)
    dec = model.continuous_decoder(2, page_size=32, max_pages=2, num_pages=2 + 2)
    with pytest.raises(ValueError, match="max_pages"):
        dec.admit(0, PROMPTS[0], 64)  # 7 + 64 > 2 * 32
    big = model.continuous_decoder(2, page_size=32, max_pages=8)
    with pytest.raises(ValueError, match="sequence length"):
        big.admit(0, PROMPTS[0], 128)  # 7 + 128 > 128
    dec.admit(0, PROMPTS[2], 20)  # 33 tokens: two pages, the pool is empty
    state = (dec.state.pos.clone(), dec.state.block_table.clone(), dec.tok.clone())
    with pytest.raises(RuntimeError, match="4 pages"):
        dec.admit(1, PROMPTS[0], 4)
    assert dec.rows[1] is None and torch.equal(dec.state.pos, state[0]) and torch.equal(dec.state.block_table, state[1])
    dec.release(0)
    dec.admit(0, PROMPTS[0], 40)  # 7 tokens: one page; position 32 needs a second
    dec.admit(1, PROMPTS[1], 4)  # takes the last page
    for _ in range(25):
        dec.step()
    state = (dec.state.pos.clone(), dec.tok.clone())
    with pytest.raises(RuntimeError, match="4 pages"):
        dec.step()
    assert torch.equal(dec.state.pos, state[0]) and torch.equal(dec.tok, state[1]) and dec.rows[0].steps == 25
    with pytest.raises(ValueError, match="holds a request"):
        dec.admit(0, PROMPTS[0], 4)
